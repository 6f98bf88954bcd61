#!/usr/bin/env python3
"""Generate tests/golden/hier/hier_*.npz by running the REAL reference (numpy backend, fp64) on its nonstationary model: a
``HierarchicalParameter`` length scale inside ``Isotropy`` (gp/hyperparameter/experimental/hierarchical.py,
gp/deformation/isotropy.py:60-89).

Run in the build container only (it needs the reference's sources on PYTHONPATH, which never travel):

    PYTHONPATH=<reference>/src PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_nonstationary.py

Nothing from the reference is copied: this script *imports* MuyGPyS, feeds it seeded inputs, and stores inputs and
outputs as data.  Import shims as in make_golden.py: package metadata for the un-installed dist and a stub
``bayes_opt`` module (importing the reference's ``optimize`` package needs it; it is never called here).

Each fixture holds the inputs (features, targets, indices, knots, knot values, the models as a JSON string in ``meta``)
and the reference's outputs: the ``(b,)`` scales of the hierarchical parameter, ``Kin`` (unperturbed), ``Kcross``,
``mean``, ``var_unscaled``, the analytic ``sigma_sq``, and the objective values ``obj_lool`` / ``obj_mse`` at two
knot-value vectors (``probes``).  The objective values come from the reference's OWN objective module
(``optimize.objective.make_loo_crossval_fn`` with ``batch_features=``): it imports under the shims.
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
from MuyGPyS.gp.deformation import F2, Isotropy, l2  # noqa: E402
from MuyGPyS.gp.hyperparameter import AnalyticScale, Parameter, VectorParameter  # noqa: E402
from MuyGPyS.gp.hyperparameter.experimental import HierarchicalParameter  # noqa: E402
from MuyGPyS.gp.kernels import RBF, Matern  # noqa: E402
from MuyGPyS.gp.noise import HomoscedasticNoise  # noqa: E402
from MuyGPyS.gp.tensors import batch_features_tensor  # noqa: E402
from MuyGPyS.optimize.loss import lool_fn, mse_fn  # noqa: E402
from MuyGPyS.optimize.objective import make_loo_crossval_fn  # noqa: E402

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hier")  # (out of the forward-fixture glob)

CASES = {
    "hier_rbf_F2": dict(seed=301, kernel="rbf", metric="F2", noise=1e-2, higher="rbf",
                        knot_values=[0.08, 0.15, 0.1, 0.22, 0.12],
                        probes=[[0.1, 0.12, 0.11, 0.2, 0.15], [0.15, 0.09, 0.18, 0.1, 0.22]]),
    "hier_m15_l2": dict(seed=302, kernel="matern15", metric="l2", noise=1e-2, higher="matern05",
                        knot_values=[0.12, 0.3, 0.1, 0.2, 0.4],
                        probes=[[0.2, 0.25, 0.15, 0.18, 0.3], [0.1, 0.4, 0.28, 0.12, 0.2]]),
}
N, D, K, B, KNOTS = 400, 2, 8, 50, 5
BOUNDS = (0.02, 1.0)


def knn_indices(X, Q, k):
    d2 = ((Q[:, None, :] - X[None, :, :]) ** 2).sum(-1)
    return np.argsort(d2, axis=1, kind="stable")[:, 1:k + 1]  # (the query is a table row: drop it)


def build(c, knots, values):
    higher = RBF() if c["higher"] == "rbf" else Matern(smoothness=Parameter(0.5))
    hp = HierarchicalParameter(knots, VectorParameter(*[Parameter(float(v), BOUNDS) for v in values]), higher)
    deformation = Isotropy(l2 if c["metric"] == "l2" else F2, length_scale=hp)
    kernel = RBF(deformation=deformation) if c["kernel"] == "rbf" else Matern(smoothness=Parameter(1.5), deformation=deformation)
    return MuyGPS(kernel=kernel, noise=HomoscedasticNoise(c["noise"]), scale=AnalyticScale())


def make_case(name, c):
    rng = np.random.default_rng(c["seed"])
    X = rng.uniform(size=(N, D))
    # smoothness varies across the domain: fast oscillation on the left, slow on the right
    y = np.sin(2 * np.pi * (1.0 + 6.0 * (1.0 - X[:, 0]) ** 2) * X[:, 0]) * np.cos(2.0 * X[:, 1]) + 0.05 * rng.normal(size=N)
    # four knots near the corners and one in the middle: the batch lies inside their hull, where the higher-level
    # posterior mean of positive knot values stays positive
    knots = np.array([[0.05, 0.05], [0.95, 0.05], [0.05, 0.95], [0.95, 0.95], [0.5, 0.5]]) + 0.02 * rng.uniform(size=(KNOTS, D))
    batch_idx = np.sort(rng.choice(N, size=B, replace=False)).astype(np.int64)
    nn_idx = knn_indices(X, X[batch_idx], K).astype(np.int64)
    m = build(c, knots, c["knot_values"])
    cross, pair, y_b, y_nn = m.make_train_tensors(batch_idx, nn_idx, X, y)
    bf = batch_features_tensor(X, batch_idx)
    scales = m.kernel.deformation.length_scale(bf)
    Kin, Kc = m.kernel(pair, batch_features=bf), m.kernel(cross, batch_features=bf)
    mean = m.posterior_mean(Kin, Kc, y_nn)
    var_unscaled = m.get_opt_var_fn()(Kin, Kc)
    sigma_sq = np.asarray(m.scale.get_opt_fn(m)(Kin, y_nn), dtype=np.float64).reshape(-1)
    names = m.get_opt_params()[0]
    assert list(names) == [f"length_scale{i}" for i in range(KNOTS)], names
    obj = {}
    for lname, lfn in (("lool", lool_fn), ("mse", mse_fn)):
        fn = make_loo_crossval_fn(lfn, m.kernel.get_opt_fn(), m.get_opt_mean_fn(), m.get_opt_var_fn(), m.scale.get_opt_fn(m),
                                  pair, cross, y_nn, y_b, batch_features=bf)
        obj[lname] = np.array([float(fn(**{n: float(v) for n, v in zip(names, p)})) for p in c["probes"]])
    meta = dict(c, name=name, N=N, d=D, k=K, b=B, knot_count=KNOTS, bounds=list(BOUNDS), objective="reference objective module")
    out = dict(features=X, targets=y, batch_idx=batch_idx, nn_idx=nn_idx, knots=knots, knot_values=np.array(c["knot_values"]),
               scales=np.asarray(scales), Kin=Kin, Kcross=Kc, mean=mean, var_unscaled=var_unscaled, sigma_sq=sigma_sq,
               batch_targets=y_b, probes=np.array(c["probes"]), obj_lool=obj["lool"], obj_mse=obj["mse"],
               meta=np.array(json.dumps(meta)))
    for values in [c["knot_values"], *c["probes"]]:
        at = build(c, knots, values).kernel.deformation.length_scale(bf)
        assert np.all(np.asarray(at) > 0), ("the fixture needs positive scales", values, np.min(at))
    os.makedirs(HERE, exist_ok=True)
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **out)
    print(f"{name}: {os.path.getsize(path) / 1024:.0f} kB; scales in [{np.min(scales):.3f}, {np.max(scales):.3f}]; "
          f"obj lool {obj['lool']}, mse {obj['mse']}")


if __name__ == "__main__":
    for name, case in CASES.items():
        make_case(name, case)
