"""CPU: the entries with a length scale per neighbourhood (mgp_posterior_ns_generic_*, mgp_posterior_ns_large_*;
include/muygpys_hip.h) -- the status of every refused or empty call in the documented order, decided BEFORE any HIP call
-- and the ``ValueError`` of every consumer of a ``KernelSpec`` that does not serve ``length_scale_batch``, as far as it
is raised without a launch; the hierarchical parameter's host-side contract; the compiler's record of the four kernels.

One rule is violated per row, starting from arguments that would launch.  Host buffers stand in for device pointers:
nothing dereferences them before the status is decided.  No row here reaches a launch."""

import ctypes as C
import json
import os

import numpy as np
import pytest

from muygpys_amd import _lib

OK, EINVAL, EUNSUPPORTED = 0, -1, -2
ES = {"f32": 4, "f64": 8}
INT_MAX, INT64_MAX = 2**31 - 1, 2**63 - 1

ENTRIES = {
    "posterior_ns_generic": "fq fn d bi ni b k tg R tb nm eps nd kid mid lsb lsc mean var yk info st",
    "posterior_ns_large": "fq fn d bi ni b k tg R tb nm eps nd kid mid lsb lsc mean var yk info ws wsb st",
}
NUMBERS = dict(d=4, b=3, k=5, R=1, tb=0, nm=0, eps=1e-3, kid=2, mid=0, lsc=1, wsb=1 << 40)
OPTIONAL = ("nd", "st", "bi", "yk", "info")
REQUIRED = "fq fn tg ni lsb mean var"
BUF = (C.c_double * 64)()
PTR = C.addressof(BUF)
assert PTR % 16 == 0


def status(entry, suf, **changes):
    names = ENTRIES[entry].split()
    args = {n: NUMBERS[n] if n in NUMBERS else (None if n in OPTIONAL else PTR) for n in names}
    unknown = set(changes) - set(names)
    assert not unknown, (entry, unknown)
    args.update(changes)
    return getattr(_lib.load(), f"mgp_{entry}_{suf}")(*[args[n] for n in names])


def rows_of(entry):
    names = ENTRIES[entry].split()
    large = entry.endswith("large")
    rows = [("b < 0", dict(b=-1), EINVAL), ("k < 1", dict(k=0), EINVAL), ("d < 1", dict(d=0), EINVAL), ("R < 1", dict(R=0), EINVAL)]
    rows += [(f"{p} NULL", {p: None}, EINVAL) for p in REQUIRED.split()]
    rows += [(f"kernel id {i}", dict(kid=i), EINVAL) for i in (-1, 6, 99)]
    rows += [(f"metric id {i}", dict(mid=i), EINVAL) for i in (-1, 2)]
    rows += [(f"noise mode {i}", dict(nm=i), EINVAL) for i in (-1, 3)]
    rows += [(f"noise mode {i} without noise_dev", dict(nm=i, nd=None), EINVAL) for i in (1, 2)]
    rows += [(f"ls_count {i} at d = 4", dict(lsc=i), EINVAL) for i in (0, 2, 5)]
    rows.append(("the general-nu id", dict(kid=5), EUNSUPPORTED))
    rows.append(("the general-nu id, length_scale_batch NULL", dict(kid=5, lsb=None), EINVAL))
    rows.append(("the general-nu id, outputs NULL", dict(kid=5, mean=None), EINVAL))
    if large:
        rows.append(("the general-nu id, workspace NULL", dict(kid=5, ws=None), EINVAL))
        rows.append(("k + 1 + R = 1025", dict(k=1023), EUNSUPPORTED))
        rows.append(("k + 1 + R = 1025 by responses", dict(k=1008, R=16), EUNSUPPORTED))
        rows.append(("k + 1 + R = 1025, length_scale_batch NULL", dict(k=1023, lsb=None), EINVAL))
        rows.append(("k = INT_MAX", dict(k=INT_MAX, wsb=INT64_MAX), EUNSUPPORTED))
        rows.append(("k = INT_MAX, a workspace of 1 TiB", dict(k=INT_MAX), EINVAL))
        rows.append(("workspace NULL", dict(ws=None), EINVAL))
        rows.append(("workspace misaligned", dict(ws=PTR + 8), EINVAL))
        rows.append(("k + 1 + R = 1025, workspace misaligned", dict(k=1023, ws=PTR + 4), EINVAL))
    else:
        rows.append(("a system beyond LDS", dict(k=1000), EUNSUPPORTED))
        rows.append(("a system beyond LDS, length_scale_batch NULL", dict(k=1000, lsb=None), EINVAL))
        rows.append(("k = INT_MAX", dict(k=INT_MAX), EUNSUPPORTED))
    nothing = {n: None for n in names if n not in NUMBERS}
    rows.append(("empty batch, all pointers NULL", dict(b=0, **nothing, **({"wsb": 0} if large else {})), OK))
    rows.append(("empty batch, ids not looked at", dict(b=0, **nothing, kid=99, mid=7, nm=8, lsc=9), OK))
    rows.append(("empty batch, k < 1", dict(b=0, k=0), EINVAL))
    return rows


GRID = [(e, n, ch, want) for e in ENTRIES for n, ch, want in rows_of(e)]


@pytest.mark.parametrize("suf", ["f32", "f64"])
@pytest.mark.parametrize("entry, name, changes, want", GRID, ids=[f"{e}: {n}" for e, n, _, _ in GRID])
def test_status_of_refused_and_empty_calls(entry, name, changes, want, suf):
    assert status(entry, suf, **changes) == want


@pytest.mark.parametrize("suf", ["f32", "f64"])
def test_lds_limit_is_the_scalar_entrys(suf):
    """The first nn_count the LDS entry refuses is mgp_max_nn_count + 1 (the carve of the scalar launch: nothing added)."""
    es = ES[suf]
    for R in (1, 3):
        limit = _lib.load().mgp_max_nn_count(es, R)
        assert status("posterior_ns_generic", suf, k=limit + 1, R=R) == EUNSUPPORTED


@pytest.mark.parametrize("suf", ["f32", "f64"])
def test_workspace_one_byte_short_of_a_slab(suf):
    es = ES[suf]
    for k, R in ((5, 1), (200, 1), (1022, 1), (1007, 16)):
        slab = _lib.load().mgp_large_workspace_bytes(es, k, R, 1)
        assert status("posterior_ns_large", suf, k=k, R=R, wsb=slab - 1) == EINVAL, (k, R)


def test_parameter_lists_are_the_gen_entries_with_two_substitutions():
    from muygpys_amd import _abi

    text = open(_abi.HEADER).read()

    def params(name):
        start = text.index(f"int {name}(")
        decl = " ".join(text[start:text.index(");", start)].split())
        return [p.strip() for p in decl[decl.index("(") + 1:].split(",")]

    for fam in ("generic", "large"):
        for suf in ("f32", "f64"):
            gen, ns = params(f"mgp_posterior_gen_{fam}_{suf}"), params(f"mgp_posterior_ns_{fam}_{suf}")
            swapped = [p.replace("double smoothness", "int kernel_id").replace("* length_scale", "* length_scale_batch") for p in gen]
            assert ns == swapped, (fam, suf)
    assert "hierarchical.py" in text and "isotropy.py:60-89" in text  # (the reference functions replaced)


def test_no_spills_no_scratch():
    path = os.path.join(os.path.dirname(_lib.LIB_PATH), "kernel_resources.json")
    with open(path) as f:
        res = json.load(f)
    mine = {n: r for n, r in res.items() if "_ns_kernel" in n}
    assert len(mine) == 4, sorted(mine)  # two families, two float widths
    for name, r in mine.items():
        assert r["VGPRs Spill"] == 0, (name, r)
        assert r["ScratchSize [bytes/lane]"] == 0, (name, r)
        assert r["LDS Size [bytes/block]"] == 0, (name, r)  # (no static LDS next to the carve of the scalar launch)


# ---- every other consumer of a KernelSpec refuses the field (checked before the tensors are looked at) -----------------
def _ns_spec(**kw):
    import torch

    from muygpys_amd.fused import KernelSpec

    return KernelSpec("matern15", "l2", 1.0, 1e-3, length_scale_batch=torch.ones(4), **kw)


def test_other_consumers_refuse_the_field():
    import torch

    from muygpys_amd import autograd, distributed, fused

    spec = _ns_spec()
    X, y = torch.zeros((8, 2)), torch.zeros(8)
    bi, ni = torch.arange(4), torch.zeros((4, 3), dtype=torch.int64)
    calls = [
        lambda: fused.loocv_partials(spec, X, y, bi, ni),
        lambda: fused.loocv_value_and_grad(spec, X, y, bi, ni),
        lambda: fused.class_value_and_grad(spec, X, torch.zeros((8, 2)), bi, ni),
        lambda: fused.fast_coefficients(spec, X, y, ni),
        lambda: fused.fast_coefficients(spec, X, y, ni, fused=False),
        lambda: fused.fast_posterior_mean(spec, X, X, bi, ni, torch.zeros((8, 3)), bi),
        lambda: autograd.posterior(spec, X, X, bi, ni, y),
        lambda: distributed.hip_local_partials(spec, X, y, bi, ni),
    ]
    for i, call in enumerate(calls):
        with pytest.raises(ValueError, match="length_scale_batch"):
            call()
        assert i >= 0
    with pytest.raises(ValueError, match="length_scale_batch"):
        fused.posterior_mean_var(_ns_spec(), X, X, bi, ni, y, path="rhs")
    spec_gen = _ns_spec()
    spec_gen.kernel, spec_gen.smoothness = "matern_gen", 1.3
    with pytest.raises(ValueError, match="length_scale_batch"):
        fused.posterior_mean_var(spec_gen, X, X, bi, ni, y)


def test_length_scale_tensor_keeps_its_error():
    import torch

    from muygpys_amd.fused import _length_scale_tensor

    with pytest.raises(ValueError, match="must have final dimension size of 3"):
        _length_scale_tensor([1.0, 2.0, 3.0], 4, torch.zeros((2, 4)))


# ---- the hierarchical parameter, host side -----------------------------------------------------------------------------
def _hier(values=(0.5, 1.0, 2.0), bounds=(0.1, 5.0)):
    from muygpys_amd.gp.hyperparameter import Parameter, VectorParameter
    from muygpys_amd.gp.hyperparameter.experimental import HierarchicalParameter
    from muygpys_amd.gp.kernels import RBF

    knots = np.array([[0.1, 0.1], [0.9, 0.2], [0.5, 0.8]])
    return HierarchicalParameter(knots, VectorParameter(*[Parameter(v, bounds) for v in values]), RBF())


def test_hierarchical_parameter_contract():
    from muygpys_amd.gp.deformation import Isotropy, l2
    from muygpys_amd.gp.hyperparameter import Parameter, VectorParameter
    from muygpys_amd.gp.hyperparameter import experimental as E
    from muygpys_amd.gp.kernels import RBF, Matern
    from muygpys_amd.gp.muygps import MuyGPS

    assert E.HierarchicalParam is E.HierarchicalParameter and E.NamedHierarchicalParam is E.NamedHierarchicalParameter
    knots = E.sample_knots(feature_count=3, knot_count=7)
    assert knots.shape == (7, 3) and knots.min() >= 0.0 and knots.max() <= 1.0
    hp = _hier()
    with pytest.raises(NotImplementedError):
        hp(None)
    with pytest.raises(NotImplementedError):
        hp.get_bounds()
    assert not hp.fixed()
    with pytest.raises(ValueError, match="same length"):
        E.HierarchicalParameter(np.zeros((2, 2)), VectorParameter(Parameter(1.0)), RBF())
    iso = Isotropy(l2, length_scale=hp)
    assert isinstance(iso.length_scale, E.NamedHierarchicalParameter) and iso.length_scale.name() == "length_scale"
    model = MuyGPS(kernel=Matern(smoothness=Parameter(1.5), deformation=iso))
    names, x0, bounds = model.get_opt_params()
    assert list(names) == ["length_scale0", "length_scale1", "length_scale2"]
    np.testing.assert_array_equal(x0, [0.5, 1.0, 2.0])
    np.testing.assert_array_equal(bounds, [[0.1, 5.0]] * 3)
    np.testing.assert_array_equal(iso.length_scale.knot_values(), [0.5, 1.0, 2.0])
    with pytest.raises(ValueError, match="batch_features"):
        model.kernel(np.zeros((2, 3, 3)))  # evaluated without batch_features=
    # anything that is neither a scalar nor a hierarchical parameter: the error Isotropy has always raised
    with pytest.raises(ValueError, match="Expected ScalarParam type for length_scale"):
        Isotropy(l2, length_scale=1.0)


def test_analytic_gradient_refuses_a_hierarchical_model_by_type():
    from muygpys_amd.gp.deformation import Isotropy, l2
    from muygpys_amd.gp.kernels import RBF
    from muygpys_amd.gp.muygps import MuyGPS
    from muygpys_amd.optimize import L_BFGS_B_optimize

    model = MuyGPS(kernel=RBF(deformation=Isotropy(l2, length_scale=_hier())))
    with pytest.raises(ValueError, match="hierarchical"):
        # (refused before the tensors are looked at: placeholders suffice)
        L_BFGS_B_optimize(model, None, None, None, None, batch_features=None, analytic_gradient=True)
