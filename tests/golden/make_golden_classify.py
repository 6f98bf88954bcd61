#!/usr/bin/env python3
"""Generate tests/golden/classify/*.npz by running the REAL reference's classification path (numpy backend, fp64).

Run in the build container only, with the same shims and run line as make_golden.py:

    PYTHONPATH=/root/reference/src PYTHONDONTWRITEBYTECODE=1 \\
        python tests/golden/make_golden_classify.py

Nothing from the reference is copied: this script *imports* MuyGPyS, feeds it seeded Gaussian mixtures and stores
inputs and outputs as data.  Per case:
  features / labels (one-hot, the encoding in ``meta``) / class_ids            the training table
  batch_indices / batch_nn_indices / mean                                      the LOOCV batch and its posterior means
  cross_entropy / mse                                                          cross_entropy_fn, mse_fn on those means
  probes / probe_cross_entropy / probe_mse                                     the objective of make_loo_crossval_fn
                                                                               at several length scales (values are
                                                                               the NEGATIVE loss, as the drivers see it)
  test_features / test_labels / test_nn_indices / predictions / nonconstant    classify_any and its agreement mask
and, for the two-class case, from classify_two_class_uq / train_two_class_interval / make_masks / do_uq:
  uq_means / uq_variances, cutv / alpha / beta (the curves of train_two_class_interval on its grid, recomputed here
  from the reference's own means and variances and checked against its cutoffs), cutoffs, masks, uq_accuracy / uq.

The generator asserts, per case, what the tests rely on: the non-constant share lies strictly between 10 % and 90 %;
at most 1 % of the predicted rows are argmax near-ties (top two means within 2 rtol (|m| + rms), rtol = 1e-3, the fp32
tolerance); every cutoff is an interior grid point and a strict minimum in the sense written at ``check_cutoffs``.
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

from MuyGPyS.examples.classify import classify_any  # noqa: E402
from MuyGPyS.examples.two_class_classify_uq import (  # noqa: E402
    classify_two_class_uq, do_uq, example_lambdas, make_masks, train_two_class_interval)
from MuyGPyS.gp import MuyGPS  # noqa: E402
from MuyGPyS.gp.deformation import Anisotropy, Isotropy, l2  # noqa: E402
from MuyGPyS.gp.hyperparameter import FixedScale, Parameter, VectorParameter  # noqa: E402
from MuyGPyS.gp.kernels import Matern  # noqa: E402
from MuyGPyS.gp.noise import HomoscedasticNoise  # noqa: E402
from MuyGPyS.neighbors import NN_Wrapper  # noqa: E402
from MuyGPyS.optimize import L_BFGS_B_optimize  # noqa: E402
from MuyGPyS.optimize.loss import cross_entropy_fn, mse_fn  # noqa: E402

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "classify")  # (out of the forward-fixture glob)
MAX_BYTES = 150_000  # the make_golden.py rule
NEAR_TIE_RTOL = 1e-3


def model(ls, noise):
    if np.ndim(ls) == 1:
        dfm = Anisotropy(l2, length_scale=VectorParameter(*[Parameter(float(v), (1e-3, 1e3)) for v in ls]))
    else:
        dfm = Isotropy(l2, length_scale=Parameter(float(ls), (1e-3, 1e3)))
    return MuyGPS(kernel=Matern(smoothness=Parameter(1.5), deformation=dfm), noise=HomoscedasticNoise(noise),
                  scale=FixedScale())


def mixture(rng, n, classes, d, sep):
    centres = rng.normal(size=(classes, d)) * sep
    ids = rng.integers(0, classes, size=n)
    return centres[ids] + rng.normal(size=(n, d)), ids, centres


def near_ties(mean, rtol):
    rms = float(np.sqrt(np.mean(mean**2)))
    top = np.sort(mean, axis=1)[:, ::-1]
    return (top[:, 0] - top[:, 1]) <= 2.0 * rtol * (np.abs(top[:, 0]) + rms)


def check_cutoffs(cutv, alpha, beta, correct_count, incorrect_count, cutoffs):
    """alpha and beta are step functions of the cutoff (means of booleans over the batch), so an objective is constant
    between two consecutive jumps and ``argmin`` returns the FIRST grid point of its lowest plateau.  "Strict minimum"
    therefore means: that plateau is interior (its value lies strictly below the objective at both ends of the grid),
    it is the only plateau with that value (the minimal grid points form one contiguous run), and the stored cutoff is
    the reference's own.  The first point of a plateau is a jump |mean| / sqrt(variance) of one sample: a result that
    agrees with the reference within the tolerances moves it by at most one grid step."""
    for j, f in enumerate(example_lambdas):
        i = int(f(alpha, beta, correct_count, incorrect_count))
        assert cutv[i] == cutoffs[j], (j, cutv[i], cutoffs[j])
        w = (1, 2, 4, 10)[j] if j < 4 else None
        obj = w * alpha + beta if w is not None else incorrect_count * alpha + correct_count * beta
        lowest = np.where(obj == obj[i])[0]
        assert 0 < i < len(cutv) - 1, (j, i)
        assert obj[i] < obj[0] and obj[i] < obj[-1] and obj[i] < obj[i - 1], (j, i)
        assert lowest[0] == i and lowest[-1] - lowest[0] + 1 == len(lowest) and lowest[-1] < len(cutv) - 1, (j, i, lowest)


def case(name, classes, encoding, aniso, k, d, sep, seed, n=480, b=110, n_test=220, noise=1e-3):
    rng = np.random.default_rng(seed)
    X, ids, centres = mixture(rng, n, classes, d, sep)
    test_ids = rng.integers(0, classes, size=n_test)
    Xt = centres[test_ids] + rng.normal(size=(n_test, d))
    lo, hi = encoding
    Y = np.full((n, classes), float(lo))
    Y[np.arange(n), ids] = float(hi)
    Yt = np.full((n_test, classes), float(lo))
    Yt[np.arange(n_test), test_ids] = float(hi)
    ls = np.linspace(0.8, 1.6, d) * 2.0 if aniso else 2.5
    m = model(ls, noise)
    nbrs = NN_Wrapper(X, k, nn_method="exact", algorithm="ball_tree")
    bi = np.sort(rng.choice(n, size=b, replace=False)).astype(np.int64)
    bni = np.asarray(nbrs.get_batch_nns(bi)[0], dtype=np.int64)
    cross, pair, y_b, y_nn = m.make_train_tensors(bi, bni, X, Y)
    mean = m.posterior_mean(m.kernel(pair), m.kernel(cross), y_nn)
    out = dict(features=X, labels=Y, class_ids=ids, batch_indices=bi, batch_nn_indices=bni, mean=mean,
               cross_entropy=np.float64(cross_entropy_fn(mean, y_b)), mse=np.float64(mse_fn(mean, y_b)))
    # objective probes (optimize/objective.py:20-105) at trial length scales
    factors = (0.5, 0.8, 1.0, 1.7)
    if aniso:
        probes = [{f"length_scale{i}": float(f * v) for i, v in enumerate(ls)} for f in factors]
    else:
        probes = [{"length_scale": float(f * ls)} for f in factors]
    for lname, lfn in (("cross_entropy", cross_entropy_fn), ("mse", mse_fn)):
        obj = L_BFGS_B_optimize.make_obj_fn(m, y_b, y_nn, cross, pair, loss_fn=lfn)
        out["probe_" + lname] = np.array([float(obj(**p)) for p in probes])
    # prediction with the agreement shortcut (examples/classify.py:537-607)
    tni = np.asarray(nbrs.get_nns(Xt)[0], dtype=np.int64)
    pred, _ = classify_any(m, Xt, X, nbrs, Y)
    col0 = Y[tni, 0]
    nonconstant = col0.max(axis=1) != col0.min(axis=1)
    share = float(nonconstant.mean())
    assert 0.10 < share < 0.90, (name, share)
    ties = float(near_ties(pred, NEAR_TIE_RTOL).mean())
    assert ties <= 0.01, (name, ties)
    assert float(near_ties(mean, NEAR_TIE_RTOL).mean()) <= 0.01, name
    out.update(test_features=Xt, test_labels=Yt, test_nn_indices=tni, predictions=pred, nonconstant=nonconstant)
    meta = dict(name=name, classes=classes, encoding=[lo, hi], aniso=aniso, k=k, d=d, kernel="matern15", metric="l2",
                length_scale=[float(v) for v in ls] if aniso else float(ls), noise=noise, probes=probes,
                nonconstant_share=share, near_tie_share=ties, accuracy=float((pred.argmax(1) == test_ids).mean()))
    if classes == 2 and (lo, hi) == (-1, 1):
        means, variances, _ = classify_two_class_uq(m, Xt, X, nbrs, Y)
        signed = 2 * ids - 1  # class labels in {-1, 1}, as train_two_class_interval compares them
        cutoffs = train_two_class_interval(m, bi, bni, X, Y, signed, example_lambdas)
        # the curves behind those cutoffs (two_class_classify_uq.py:467-514), from the reference's own regression
        from MuyGPyS.examples.from_indices import regress_from_indices

        bmean, bvar = regress_from_indices(m, bi, bni, X, X, Y)
        correct = (2 * np.argmax(bmean, axis=1) - 1) == signed[bi]
        cutv = np.linspace(0.01, 20, 1999)
        sd = np.sqrt(bvar)
        inside = (bmean[None, :, 1] - cutv[:, None] * sd[None, :] < 0.0) & (bmean[None, :, 1] + cutv[:, None] * sd[None, :] > 0.0)
        alpha, beta = 1.0 - inside[:, ~correct].mean(axis=1), inside[:, correct].mean(axis=1)
        check_cutoffs(cutv, alpha, beta, int(correct.sum()), int((~correct).sum()), cutoffs)
        masks = make_masks(means, cutoffs, variances, 0.0)
        accuracy, uq = do_uq(means, Yt, masks)
        out.update(uq_means=means, uq_variances=variances, batch_variance=bvar, cutv=cutv, alpha=alpha, beta=beta,
                   correct_mask=correct, cutoffs=cutoffs, masks=masks, uq_accuracy=np.float64(accuracy), uq=uq)
    out["meta"] = np.array(json.dumps(meta))
    os.makedirs(HERE, exist_ok=True)
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **{k_: np.asarray(v) for k_, v in out.items()})
    size = os.path.getsize(path)
    assert size <= MAX_BYTES, (name, size)
    print(f"{name}: {size} bytes, non-constant {share:.2f}, near ties {ties:.3f}, accuracy {meta['accuracy']:.3f}")


if __name__ == "__main__":
    case("c2_pm1_iso_k12", 2, (-1, 1), False, 12, 4, 0.9, 11)
    case("c2_01_iso_k30", 2, (0, 1), False, 30, 6, 1.3, 12)
    case("c3_pm1_aniso_k12", 3, (-1, 1), True, 12, 5, 1.2, 13)
    case("c10_pm1_iso_k30", 10, (-1, 1), False, 30, 8, 1.0, 14)
    case("c10_pm1_aniso_k12", 10, (-1, 1), True, 12, 8, 0.9, 15)
