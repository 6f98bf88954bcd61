"""The shear model without a GPU: the numpy oracle against the reference's fixtures, the C ABI's argument checks,
and the backend family's names."""

import ctypes as C
import json
import os

import numpy as np
import pytest

from tests import shear_oracle as O

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "shear")


def _load(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"))


@pytest.mark.parametrize("name", ["shear_33_k10", "shear_23_k10"])
def test_oracle_matches_every_stage(name):
    g = _load(name)
    meta = json.loads(str(g["meta"]))
    ell, eps = meta["length_scale"], meta["noise"]
    model = meta["kind"]
    mean, cov, Kin, Kc, P, tg = O.posterior(g["features"], g["targets"], g["batch_indices"], g["nn_indices"], ell, eps,
                                            model, "shear33" if model == "33" else "homoscedastic")
    for got, ref in ((Kin, g["Kin"]), (Kc, g["Kcross"]), (P, g["Kin_perturbed"]), (tg, g["batch_nn_targets"]),
                     (O.kout(ell), g["Kout"]), (mean, g["mean"]), (cov, g["variance"])):
        np.testing.assert_allclose(got, ref, rtol=1e-9, atol=1e-9 * np.abs(ref).max())


@pytest.mark.parametrize("name", ["shear_33_k50", "shear_23_k50"])
def test_oracle_matches_outputs_at_k50(name):
    g = _load(name)
    meta = json.loads(str(g["meta"]))
    model = meta["kind"]
    mean, cov, *_ = O.posterior(g["features"], g["targets"], g["batch_indices"], g["nn_indices"], meta["length_scale"],
                                meta["noise"], model, "shear33" if model == "33" else "homoscedastic")
    np.testing.assert_allclose(mean, g["mean"], rtol=1e-6, atol=1e-6 * np.abs(g["mean"]).max())
    np.testing.assert_allclose(cov, g["variance"], rtol=1e-6, atol=1e-6 * np.abs(g["variance"]).max())


def test_oracle_matches_squeezed_b1_shapes():
    g = _load("shear_b1")
    ell = float(g["length_scale"])
    cross = g["crosswise"][..., None, :]
    for got, ref in ((O.shear_33(g["pairwise"], ell), g["Kin33"]), (O.shear_33(cross, ell), g["Kcross33"]),
                     (O.shear_kin23(g["pairwise"], ell), g["Kin23"]), (O.shear_kcross23(cross, ell), g["Kcross23"])):
        assert got.shape == ref.shape
        np.testing.assert_allclose(got, ref, rtol=1e-12, atol=1e-12 * np.abs(ref).max())


def _lib():
    from muygpys_amd import _lib

    return _lib.load()


def test_shear_abi_rejects_bad_arguments_without_a_gpu():
    lib = _lib()
    buf = (C.c_double * 64)()
    idx = (C.c_int64 * 8)()
    info = (C.c_int * 1)()
    p, i = C.cast(buf, C.c_void_p), C.cast(idx, C.c_void_p)
    st = None
    # shear tensors: null pointers, bad variant, bad length scale, negative sizes
    assert lib.mgp_shear_tensor_f64(None, 1, 2, 2, 0, 1.0, p, st) == -1
    assert lib.mgp_shear_tensor_f64(p, 1, 2, 2, 0, 1.0, None, st) == -1
    assert lib.mgp_shear_tensor_f64(p, 1, 2, 2, 3, 1.0, p, st) == -1
    assert lib.mgp_shear_tensor_f32(p, 1, 2, 2, 0, 0.0, p, st) == -1
    assert lib.mgp_shear_tensor_f64(p, -1, 2, 2, 0, 1.0, p, st) == -1
    # multi-output solve
    assert lib.mgp_solve_multi_f64(None, p, p, 1, 4, 3, 1, p, p, p, info, st) == -1
    assert lib.mgp_solve_multi_f64(p, None, p, 1, 4, 3, 1, p, p, p, info, st) == -1
    assert lib.mgp_solve_multi_f64(p, p, None, 1, 4, 3, 1, p, p, p, info, st) == -1
    assert lib.mgp_solve_multi_f32(p, p, p, 1, 0, 3, 1, p, p, p, info, st) == -1
    assert lib.mgp_solve_multi_f32(p, p, p, -1, 4, 3, 1, p, p, p, info, st) == -1
    assert lib.mgp_solve_multi_f64(p, p, p, 1, 4, 3, 1, None, None, None, info, st) == -1
    # fused posterior: null pointers, in_count, noise mode, shear33 with two inputs, stride, length scale
    args = lambda **kw: [kw.get(n, v) for n, v in (
        ("fq", p), ("fn", p), ("bi", i), ("ni", i), ("b", 1), ("k", 4), ("in_", 3), ("tg", p), ("ts", 3), ("tb", 0),
        ("ls", 1.0), ("nm", 1), ("eps", 1e-3), ("mean", p), ("kk", p), ("yk", p), ("info", info), ("st", None))]
    f64 = lib.mgp_shear_posterior_f64  # (bound from the header by _lib.load, like every entry point)
    for bad in (dict(fq=None), dict(fn=None), dict(ni=None), dict(tg=None), dict(mean=None), dict(kk=None),
                dict(in_=4), dict(nm=2), dict(in_=2, nm=1), dict(ts=2), dict(ls=-1.0), dict(k=0), dict(b=-1),
                dict(eps=-1.0)):
        assert f64(*args(**bad)) == -1, bad
    # beyond the LDS capacity: unsupported, before any HIP call
    assert f64(*args(k=10_000)) == -2
    assert lib.mgp_shear_max_nn_count(8, 4) == -1 and lib.mgp_shear_max_nn_count(2, 3) == -1


def test_shear_capacity_covers_the_issue_shapes():
    lib = _lib()
    assert lib.mgp_shear_max_nn_count(8, 3) >= 50
    for es, i in ((4, 3), (4, 2), (8, 2)):
        assert lib.mgp_shear_max_nn_count(es, i) >= 64, (es, i)


def test_backend_family_exports_the_reference_names():
    from muygpys_amd._src.gp.kernels.shear import hip

    for name in ("_shear_33_fn", "_shear_Kin23_fn", "_shear_Kcross23_fn"):
        assert callable(getattr(hip, name))
    from muygpys_amd._src.gp.kernels import shear

    assert sorted(shear.__all__) == ["_shear_33_fn", "_shear_Kcross23_fn", "_shear_Kin23_fn"]


def test_functor_mirror_refuses_other_deformations():
    from muygpys_amd.gp.deformation import F2, Isotropy
    from muygpys_amd.gp.hyperparameter import ScalarParam
    from muygpys_amd.gp.kernels import ShearKernel, ShearKernel2in3out
    from muygpys_amd.gp.noise import HomoscedasticNoise, ShearNoise33

    for cls in (ShearKernel, ShearKernel2in3out):
        with pytest.raises(ValueError):
            cls(deformation=Isotropy(F2, length_scale=ScalarParam(1.0)))
    assert issubclass(ShearNoise33, HomoscedasticNoise)
