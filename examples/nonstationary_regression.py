#!/usr/bin/env python3
"""Nonstationary regression with a hierarchical length scale (the flow of the reference's
experimental/nonstationary_tutorial.ipynb) on the hip backend: a 1-D curve that oscillates fast on the left and slowly
on the right, a handful of knots whose values are the length scale there, k-NN, L-BFGS-B over the knot values, prediction.

    python examples/nonstationary_regression.py          # needs a ROCm device

The length scale of every neighbourhood is the posterior mean of a small higher-level GP over the knots, evaluated at
the batch element's features; the whole posterior is ONE fused launch with a length scale per neighbourhood.
"""

import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

from muygpys_amd import _lib
from muygpys_amd.gp import MuyGPS
from muygpys_amd.gp.deformation import Isotropy, l2
from muygpys_amd.gp.hyperparameter import AnalyticScale, Parameter, VectorParameter
from muygpys_amd.gp.hyperparameter.experimental import HierarchicalParameter
from muygpys_amd.gp.kernels import Matern
from muygpys_amd.gp.noise import HomoscedasticNoise
from muygpys_amd.gp.tensors import batch_features_tensor
from muygpys_amd.neighbors import NN_Wrapper
from muygpys_amd.optimize import L_BFGS_B_optimize
from muygpys_amd.optimize.loss import lool_fn


def curve(x, rng, noise):
    """Frequency falling from left to right: the right length scale is several times the left one."""
    return np.sin(2 * np.pi * (1.0 + 7.0 * (1.0 - x) ** 2) * x) + np.sqrt(noise) * rng.standard_normal(x.shape)


def run(seed=0, n=3000, train_step=3, nn_count=12, knot_count=4, noise=1e-3, batch_count=300, verbose=True):
    rng = np.random.default_rng(seed)
    x = np.linspace(0.0, 1.0, n)
    y = curve(x, rng, noise)
    test_mask = np.ones(n, dtype=bool)
    test_mask[::train_step] = False
    dev = torch.device("cuda")
    Xtr = torch.tensor(x[~test_mask], device=dev)[:, None]
    ytr = torch.tensor(y[~test_mask], device=dev)
    Xte = torch.tensor(x[test_mask], device=dev)[:, None]
    yte = y[test_mask]

    # knots: evenly spaced over the domain, every knot value free in (0.01, 1), all starting at 0.1
    knots = np.linspace(0.0, 1.0, knot_count)[:, None]
    knot_values = VectorParameter(*[Parameter(0.1, (0.01, 1.0)) for _ in range(knot_count)])
    # (the higher-level kernel: Matern 1/2, whose 1-D posterior mean between two knots is a positive combination of
    # their values -- positive knot values give positive length scales everywhere)
    higher = Matern(smoothness=Parameter(0.5), deformation=Isotropy(l2, length_scale=Parameter(0.5)))
    length_scale = HierarchicalParameter(knots, knot_values, higher)
    muygps = MuyGPS(
        kernel=Matern(smoothness=Parameter(2.5), deformation=Isotropy(l2, length_scale=length_scale)),
        noise=HomoscedasticNoise(noise),
        scale=AnalyticScale(),
    )
    nbrs = NN_Wrapper(Xtr, nn_count)
    batch_count = min(batch_count, Xtr.shape[0])
    batch_idx = torch.tensor(np.sort(rng.choice(Xtr.shape[0], batch_count, replace=False)), device=dev)
    batch_nn, _ = nbrs.get_batch_nns(batch_idx)
    cross, pair, y_b, y_nn = muygps.make_train_tensors(batch_idx, batch_nn, Xtr, ytr)
    batch_features = batch_features_tensor(Xtr, batch_idx)
    muygps = L_BFGS_B_optimize(muygps, y_b, y_nn, cross, pair, batch_features=batch_features, loss_fn=lool_fn)
    opt_fn = muygps.scale.get_opt_fn(muygps)
    muygps.scale._set(opt_fn(muygps.kernel(pair, batch_features=batch_features), y_nn))
    muygps._make()

    test_nn, _ = nbrs.get_nns(Xte)
    cross, pair, y_nn = muygps.make_predict_tensors(None, test_nn, Xte, Xtr, ytr)
    Kin, Kcross = muygps.kernel(pair, batch_features=Xte), muygps.kernel(cross, batch_features=Xte)
    mean = muygps.posterior_mean(Kin, Kcross, y_nn).cpu().numpy()
    served = _lib.last_kernel()
    var = muygps.posterior_variance(Kin, Kcross).cpu().numpy()
    scales = muygps.kernel.deformation.length_scale(Xte).cpu().numpy()
    out = dict(knot_values=[float(v) for v in muygps.kernel.deformation.length_scale.knot_values()],
               length_scale_left=float(scales[0]), length_scale_right=float(scales[-1]), sigma_sq=muygps.scale(),
               rmse=float(np.sqrt(np.mean((mean - yte) ** 2))),
               coverage=float(np.mean(np.abs(mean - yte) <= 1.96 * np.sqrt(var))), target_std=float(np.std(yte)),
               kernel=served)
    if verbose:
        print(out)
        print("served by", served)
    return out


if __name__ == "__main__":
    run()
