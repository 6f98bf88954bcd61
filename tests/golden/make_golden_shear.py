#!/usr/bin/env python3
"""Generate tests/golden/shear/shear_*.npz by running the REAL reference's shear model (numpy backend, fp64).

Run in the build container only, with the same shims and run line as make_golden.py:

    PYTHONPATH=/root/reference/src PYTHONDONTWRITEBYTECODE=1 \\
        python tests/golden/make_golden_shear.py

Nothing from the reference is copied: this script *imports* MuyGPyS, feeds it seeded inputs and stores
inputs and outputs as data.  Cases:
  shear_33_k10   ShearKernel + ShearNoise33, every stage (differences, Kin, Kcross, perturbed Kin, Kout,
                 mean, variance)
  shear_23_k10   ShearKernel2in3out + HomoscedasticNoise, every stage
  shear_33_k50 / shear_23_k50   outputs only
  shear_b1       the b = 1 shapes (the reference squeezes the batch dimension away)
  shear_grid     a seeded version of the reference test's 25 x 25 unit-square grid (l = 0.05, eps = 1e-4):
                 features and a GP draw of (kappa, gamma1, gamma2) targets
"""

import importlib.metadata as md
import json
import os
import sys
import types

_v = md.version
md.version = lambda n: "0.9.0" if n == "MuyGPyS" else _v(n)
_bo = types.ModuleType("bayes_opt")
_bo.BayesianOptimization = object
sys.modules["bayes_opt"] = _bo

import numpy as np  # noqa: E402

from MuyGPyS.gp import MuyGPS  # noqa: E402
from MuyGPyS.gp.deformation import DifferenceIsotropy, F2  # noqa: E402
from MuyGPyS.gp.hyperparameter import FixedScale, Parameter  # noqa: E402
from MuyGPyS.gp.kernels.experimental import ShearKernel, ShearKernel2in3out  # noqa: E402
from MuyGPyS.gp.noise import HomoscedasticNoise  # noqa: E402
from MuyGPyS.gp.noise.shear import ShearNoise33  # noqa: E402

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "shear")  # (out of the forward-fixture glob)
MAX_BYTES = 150_000  # the make_golden.py rule for stored intermediates


def model(kind, ell, eps):
    dfm = DifferenceIsotropy(F2, length_scale=Parameter(ell))
    if kind == "33":
        return MuyGPS(kernel=ShearKernel(deformation=dfm), noise=ShearNoise33(eps), scale=FixedScale())
    return MuyGPS(kernel=ShearKernel2in3out(deformation=dfm), noise=HomoscedasticNoise(eps), scale=FixedScale())


def case(name, kind, n, b, k, ell, eps, seed, stages):
    rng = np.random.default_rng(seed)
    X = rng.uniform(size=(n, 2))
    Y = rng.normal(size=(n, 3))
    bi = rng.choice(n, size=b, replace=False)
    ni = np.stack([rng.choice(np.delete(np.arange(n), i), size=k, replace=False) for i in bi])
    m = model(kind, ell, eps)
    cross, pair, nn_t = m.make_predict_tensors(np.arange(b), ni, X[bi], X, Y)
    nn_t = nn_t.swapaxes(-2, -1)
    if kind == "23":
        nn_t = nn_t[:, 1:, :]
    Kcross = m.kernel(cross)  # (b != k: the functors' shape rule applies)
    Kin = m.kernel(pair)
    mean = m.posterior_mean(Kin, Kcross, nn_t)
    var = m.posterior_variance(Kin, Kcross)
    out = dict(features=X, targets=Y, batch_indices=bi, nn_indices=ni, mean=mean, variance=var,
               Kout=np.asarray(m.kernel.Kout()),
               meta=json.dumps(dict(kind=kind, length_scale=ell, noise=eps, k=k, b=b)))
    if stages:
        out.update(crosswise=cross, pairwise=pair, Kin=Kin, Kcross=Kcross, Kin_perturbed=m.noise.perturb(Kin),
                   batch_nn_targets=nn_t)
    save(name, out)


def b1():
    rng = np.random.default_rng(7)
    k = 6
    pair = rng.normal(size=(1, k, k, 2))
    pair = pair - np.swapaxes(pair, 1, 2)
    cross = rng.normal(size=(1, k, 2))
    m33, m23 = model("33", 0.3, 1e-3), model("23", 0.3, 1e-3)
    save("shear_b1", dict(pairwise=pair, crosswise=cross, Kin33=m33.kernel(pair), Kcross33=m33.kernel(cross),
                          Kin23=m23.kernel(pair), Kcross23=m23.kernel(cross), length_scale=np.float64(0.3)))


def grid():
    from MuyGPyS._src.gp.kernels.shear.numpy import _shear_33_fn

    side, ell, eps = 25, 0.05, 1e-4
    g = np.linspace(0.0, 1.0, side)
    X = np.stack(np.meshgrid(g, g, indexing="ij"), axis=-1).reshape(-1, 2)
    n = X.shape[0]
    K = _shear_33_fn(X[:, None, :] - X[None, :, :], length_scale=ell).reshape(3 * n, 3 * n)
    L = np.linalg.cholesky(K + 1e-8 * np.mean(np.diag(K)) * np.eye(3 * n))
    y = L @ np.random.default_rng(11).normal(size=3 * n)
    Y = y.reshape(3, n).T.copy()
    save("shear_grid", dict(features=X, targets=Y, length_scale=np.float64(ell), noise=np.float64(eps)))


def save(name, arrays):
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **{k: np.asarray(v) for k, v in arrays.items()})
    size = os.path.getsize(path)
    assert size <= MAX_BYTES, (name, size)
    print(name, size, "bytes")


if __name__ == "__main__":
    case("shear_33_k10", "33", 200, 6, 10, 0.3, 1e-3, 1, stages=True)
    case("shear_23_k10", "23", 200, 6, 10, 0.3, 1e-3, 2, stages=True)
    case("shear_33_k50", "33", 400, 8, 50, 0.1, 1e-2, 3, stages=False)
    case("shear_23_k50", "23", 400, 8, 50, 0.1, 1e-2, 4, stages=False)
    b1()
    grid()
