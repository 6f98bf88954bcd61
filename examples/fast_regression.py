#!/usr/bin/env python3
"""The reference's fast-prediction workflow (docs/examples/fast_regression_tutorial.ipynb: precompute the
coefficients of every training point's neighbourhood once, then predict a test point from its closest training
point's neighbourhood) on the hip backend, at any nn_count.

    python examples/fast_regression.py --nn-count 100 --responses 3      # needs a ROCm device

The coefficient table is one fused launch and the prediction another, whatever nn_count is
(nn_count + 1 + responses <= 1024); the conventional posterior mean on the same model is printed next to it.

    python examples/fast_regression.py --smoothness 1.37 --nn-count 100 --responses 3

runs a free-smoothness Matern (the Bessel form, e.g. what an optimiser left behind) through the same two launches:
``fused.gen_fast("fused")`` is switched on for the workflow, and the library entries that served it are printed.
"""

import argparse
import contextlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

from muygpys_amd import _lib, fused
from muygpys_amd.examples.fast_posterior_mean import fast_posterior_mean_any
from muygpys_amd.gp import MuyGPS
from muygpys_amd.gp.deformation import Isotropy, l2
from muygpys_amd.gp.hyperparameter import Parameter
from muygpys_amd.gp.kernels import Matern
from muygpys_amd.gp.noise import HomoscedasticNoise
from muygpys_amd.neighbors import NN_Wrapper


def run(seed=0, train_count=20000, test_count=2000, feature_count=8, nn_count=100, responses=1, length_scale=1.5,
        noise=1e-3, dtype="float32", verbose=True, smoothness=None):
    rng = np.random.default_rng(seed)
    X = rng.uniform(size=(train_count + test_count, feature_count))
    W = rng.normal(size=(feature_count, responses))
    Y = np.sin(3.0 * X @ W) + np.sqrt(noise) * rng.normal(size=(train_count + test_count, responses))
    td, dev = getattr(torch, dtype), torch.device("cuda")
    Xtr, Xte = torch.tensor(X[:train_count], device=dev, dtype=td), torch.tensor(X[train_count:], device=dev, dtype=td)
    Ytr, Yte = torch.tensor(Y[:train_count], device=dev, dtype=td), Y[train_count:]
    if responses == 1:
        Ytr, Yte = Ytr[:, 0], Yte[:, 0]

    # smoothness None: the closed-form Matern-3/2; a number: the general-smoothness Matern on the fused kernels
    nu = 1.5 if smoothness is None else float(smoothness)
    muygps = MuyGPS(kernel=Matern(smoothness=Parameter(nu), deformation=Isotropy(l2, Parameter(length_scale))),
                    noise=HomoscedasticNoise(noise))
    nbrs = NN_Wrapper(Xtr, nn_count)
    entries, real_fn = [], _lib.fn

    def noting_fn(base, dtype_):
        if base.startswith("fast_") and base not in entries:
            entries.append(base)
        return real_fn(base, dtype_)

    _lib.fn = noting_fn
    try:
        with fused.gen_fast("fused") if smoothness is not None else contextlib.nullcontext():
            mean, coeffs, timing = fast_posterior_mean_any(muygps, Xte, Xtr, nbrs, Ytr)
    finally:
        _lib.fn = real_fn

    test_nn, _ = nbrs.get_nns(Xte)
    cross, pair, y_nn = muygps.make_predict_tensors(None, test_nn, Xte, Xtr, Ytr)
    full = muygps.posterior_mean(muygps.kernel(pair), muygps.kernel(cross), y_nn)
    out = dict(nn_count=nn_count, responses=responses, dtype=dtype, smoothness=nu, served_by=["mgp_" + e for e in entries],
               coefficients=tuple(coeffs.shape),
               rmse_fast=float(np.sqrt(np.mean((mean.cpu().numpy() - Yte) ** 2))),
               rmse_posterior=float(np.sqrt(np.mean((full.cpu().numpy() - Yte) ** 2))),
               target_std=float(np.std(Yte)), timing={k: round(v, 4) for k, v in timing.items()})
    if verbose:
        print(out)
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--nn-count", type=int, default=100)
    ap.add_argument("--responses", type=int, default=1)
    ap.add_argument("--train-count", type=int, default=20000)
    ap.add_argument("--test-count", type=int, default=2000)
    ap.add_argument("--feature-count", type=int, default=8)
    ap.add_argument("--dtype", choices=("float32", "float64"), default="float32")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--smoothness", type=float, default=None, metavar="NU",
                    help="a free Matern smoothness (0 < NU <= 30): the general-smoothness model on the fused kernels")
    a = ap.parse_args()
    run(seed=a.seed, train_count=a.train_count, test_count=a.test_count, feature_count=a.feature_count,
        nn_count=a.nn_count, responses=a.responses, dtype=a.dtype, smoothness=a.smoothness)
