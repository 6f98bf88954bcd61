#!/usr/bin/env python3
"""A classifier on the hip backend: a seeded Gaussian mixture, k-NN, the kernel's length scale trained on the
cross-entropy of a LOOCV batch -- once with ``Bayes_optimize``, once with ``L_BFGS_B_optimize`` and the analytic
gradient -- and prediction with ``classify_any``, which solves only the neighbourhoods whose labels disagree.

    python examples/classification.py          # needs a ROCm device

Prints one JSON line: the two trained length scales, their test accuracies and the share of test points that
needed the GP solve.
"""

import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

from muygpys_amd.examples.classify import classify_any
from muygpys_amd.gp import MuyGPS
from muygpys_amd.gp.deformation import Isotropy, l2
from muygpys_amd.gp.hyperparameter import FixedScale, Parameter
from muygpys_amd.gp.kernels import Matern
from muygpys_amd.gp.noise import HomoscedasticNoise
from muygpys_amd.neighbors import NN_Wrapper
from muygpys_amd.optimize import Bayes_optimize, L_BFGS_B_optimize
from muygpys_amd.optimize.loss import cross_entropy_fn


def mixture(rng, centres, n):
    ids = rng.integers(0, centres.shape[0], size=n)
    return centres[ids] + rng.normal(size=(n, centres.shape[1])), ids


def run(seed=0, classes=5, d=8, train_count=20000, test_count=5000, nn_count=20, batch_count=1500, separation=1.1,
        verbose=True):
    rng = np.random.default_rng(seed)
    centres = rng.normal(size=(classes, d)) * separation
    X, ids = mixture(rng, centres, train_count)
    Xt, test_ids = mixture(rng, centres, test_count)
    Y = -np.ones((train_count, classes))
    Y[np.arange(train_count), ids] = 1.0          # one-hot in {-1, 1}
    dev = torch.device("cuda")
    Xd, Yd, Xtd = (torch.tensor(a, device=dev) for a in (X, Y, Xt))

    def model():
        return MuyGPS(
            kernel=Matern(smoothness=Parameter(1.5), deformation=Isotropy(l2, length_scale=Parameter(1.0, (0.2, 20.0)))),
            noise=HomoscedasticNoise(1e-3), scale=FixedScale(),
        )

    nbrs = NN_Wrapper(Xd, nn_count)
    batch_idx = torch.tensor(np.sort(rng.choice(train_count, batch_count, replace=False)), device=dev)
    batch_nn, _ = nbrs.get_batch_nns(batch_idx)
    out = dict(classes=classes, train_count=train_count, test_count=test_count, nn_count=nn_count)
    for name in ("bayes", "lbfgs_analytic"):
        m = model()
        cross, pair, y_b, y_nn = m.make_train_tensors(batch_idx, batch_nn, Xd, Yd)
        if name == "bayes":
            m = Bayes_optimize(m, y_b, y_nn, cross, pair, loss_fn=cross_entropy_fn, random_state=seed, init_points=3, n_iter=10)
        else:
            m = L_BFGS_B_optimize(m, y_b, y_nn, cross, pair, loss_fn=cross_entropy_fn, analytic_gradient=True)
        pred, timing = classify_any(m, Xtd, Xd, nbrs, Yd)
        out[name] = dict(length_scale=float(m.kernel.deformation.length_scale()),
                         accuracy=float((pred.argmax(dim=1).cpu().numpy() == test_ids).mean()))
    labels0 = Yd[nbrs.get_nns(Xtd)[0], 0]
    out["solved_share"] = float((labels0.max(dim=1).values != labels0.min(dim=1).values).double().mean())
    if verbose:
        print(json.dumps(out))
    return out


if __name__ == "__main__":
    run()
