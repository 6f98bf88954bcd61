"""The fast-posterior-mean workflow on the hip backend.

Mirrors the prediction half of the reference's ``MuyGPyS.examples.fast_posterior_mean`` -- ``make_fast_regressor``
(examples/fast_posterior_mean.py:39-87), ``make_fast_multivariate_regressor`` (:90-135) and
``fast_posterior_mean_any`` (:317-400) -- with the reference's signatures over device tensors and
:class:`muygpys_amd.neighbors.NN_Wrapper`.  ``do_fast_posterior_mean`` (training included) is not mirrored.

On device tensors the tensors of the workflow are lazy handles, so that for any ``nn_count`` (and response count, with
``nn_count + 1 + response_count <= 1024``)

* the coefficient table comes from ONE fused launch per model (``mgp_fast_coefficients_*`` /
  ``mgp_fast_coefficients_any_*``): nothing of size ``(train_count, nn_count, nn_count)`` is formed;
* the prediction is ONE launch of the fused prediction kernel per model (``mgp_fast_posterior_mean_*``), which picks
  each test point's coefficient row itself.

Host (numpy) arrays, with a model whose ``_backend_*`` callables take them and a neighbour lookup that serves them, go
through the model's own callables on materialised tensors, in the reference's order.

A multivariate model is any object with a ``models`` sequence of :class:`muygpys_amd.gp.MuyGPS`, one per response
column (the reference's ``MultivariateMuyGPS``): column ``i`` of the coefficients and of the prediction comes from
``models[i]`` and its hyper-parameters.
"""

from __future__ import annotations

from time import perf_counter
from typing import Dict, Tuple

import numpy as np
import torch

from muygpys_amd import lazy as _lazy
from muygpys_amd import lazy_eval as _lazy_eval
from muygpys_amd.gp import tensors as _tensors


def _on_device(*xs) -> bool:
    return all(isinstance(x, torch.Tensor) and x.is_cuda for x in xs)


def _arange(n: int, like):
    return torch.arange(n, device=like.device) if isinstance(like, torch.Tensor) else np.arange(n)


def _sync(like) -> None:
    if _on_device(like):
        torch.cuda.synchronize()


def fast_nn_update(nn_indices):
    """gp/tensors.py:52-90: each point in front of its own neighbours, the farthest dropped -- on the device
    (:func:`muygpys_amd.gp.tensors.fast_nn_update`) or, for a host array, in numpy."""
    if _on_device(nn_indices):
        return _tensors.fast_nn_update(nn_indices)
    nn_indices = np.asarray(nn_indices)
    me = np.arange(nn_indices.shape[0], dtype=nn_indices.dtype)
    return np.concatenate((me[:, None], nn_indices[:, :-1]), axis=1)


def _self_including_neighbourhoods(nbrs_lookup, train_features):
    nn_indices, _ = nbrs_lookup.get_batch_nns(_arange(train_features.shape[0], train_features))
    return fast_nn_update(nn_indices)


def _coefficients(muygps, train_features, train_targets, nn_indices):
    """``muygps.fast_coefficients`` of the self-including neighbourhoods: on lazy handles where the tables are on the
    device (one fused launch), on the reference's tensors otherwise."""
    on_device = _on_device(train_features, train_targets)
    pairwise = muygps.kernel.deformation.pairwise_tensor(train_features, nn_indices, **({"lazy": True} if on_device else {}))
    nn_targets = _lazy.LazyTargets(train_targets, nn_indices) if on_device else train_targets[nn_indices]
    return muygps.fast_coefficients(muygps.kernel(pairwise), nn_targets)


def make_fast_regressor(muygps, nbrs_lookup, train_features, train_targets):
    """examples/fast_posterior_mean.py:39-87: the precomputed coefficients ``(train_count, nn_count[, response_count])``
    and the self-including neighbour table ``(train_count, nn_count)`` of a (possibly trained) ``MuyGPS``."""
    nn_indices = _self_including_neighbourhoods(nbrs_lookup, train_features)
    return _coefficients(muygps, train_features, train_targets, nn_indices), nn_indices


def make_fast_multivariate_regressor(mmuygps, nbrs_lookup, train_features, train_targets):
    """examples/fast_posterior_mean.py:90-135: the same for a multivariate model -- one launch per model, over the
    response column with that model's hyper-parameters; coefficients ``(train_count, nn_count, response_count)``."""
    models = list(mmuygps.models)
    if train_targets.ndim != 2 or train_targets.shape[1] != len(models):
        raise ValueError(f"{len(models)} models need train_targets of shape (train_count, {len(models)})")
    nn_indices = _self_including_neighbourhoods(nbrs_lookup, train_features)
    columns = [_coefficients(m, train_features, train_targets[:, i], nn_indices) for i, m in enumerate(models)]
    stack = torch.stack if isinstance(columns[0], torch.Tensor) else np.stack
    return stack(columns, -1), nn_indices


def _is_multivariate(muygps) -> bool:
    return hasattr(muygps, "models")


def _decide_and_make_fast_regressor(muygps, nbrs_lookup, train_features, train_targets):
    make = make_fast_multivariate_regressor if _is_multivariate(muygps) else make_fast_regressor
    return make(muygps, nbrs_lookup, train_features, train_targets)


def _predict(muygps, indices, closest_set, test_features, train_features, closest_neighbor, coeffs):
    """examples/from_indices.py:93-118 (fast_posterior_mean_from_indices) for one model."""
    if _on_device(test_features, train_features, coeffs):
        crosswise = muygps.kernel.deformation.crosswise_tensor(test_features, train_features, indices, closest_set, lazy=True)
        Kcross = muygps.kernel(crosswise)
        # (the prediction kernel picks each test point's coefficient row itself: no gathered (b, k, R) copy)
        out = _lazy_eval.fast_mean(Kcross, coeffs, rows=closest_neighbor)
        return out if out is not None else muygps.fast_posterior_mean(Kcross, coeffs[closest_neighbor])
    crosswise = muygps.kernel.deformation.crosswise_tensor(test_features, train_features, indices, closest_set)
    return muygps.fast_posterior_mean(muygps.kernel(crosswise), coeffs[closest_neighbor])


def fast_posterior_mean_any(muygps, test_features, train_features, nbrs_lookup, train_targets) -> Tuple[object, object, Dict[str, float]]:
    """examples/fast_posterior_mean.py:317-400: fast posterior mean inference with a pre-trained model, univariate or
    multivariate.  Returns the predicted responses of the test points, the precomputed coefficients and the timing of
    the subroutines (``precompute``, ``agree``, ``nn``, ``pred``; the device is waited for at the end of ``precompute``
    and of ``pred``).

    ``fast_nn_update`` is applied ONCE, inside the regressor: the neighbourhood of training point ``i`` is
    ``[i, nn[i][:-1]]``, the one its coefficients were solved on.  The reference's function applies it a second time to
    the table the regressor returns (:373) and so predicts on ``[i, i, nn[i][:-2]]`` with coefficients of another
    neighbourhood; that is not copied here."""
    time_start = perf_counter()
    coeffs, nn_indices = _decide_and_make_fast_regressor(muygps, nbrs_lookup, train_features, train_targets)
    _sync(train_features)
    time_precomp = perf_counter()

    time_agree = perf_counter()
    test_neighbors, _ = nbrs_lookup.get_nns(test_features)
    time_nn = perf_counter()

    closest_neighbor = test_neighbors[:, 0]
    closest_set = nn_indices[closest_neighbor, :]
    indices = _arange(test_features.shape[0], test_features)
    if _is_multivariate(muygps):
        columns = [_predict(m, indices, closest_set, test_features, train_features, closest_neighbor, coeffs[:, :, i])
                   for i, m in enumerate(muygps.models)]
        stack = torch.stack if isinstance(columns[0], torch.Tensor) else np.stack
        posterior_mean = stack(columns, -1)
    else:
        posterior_mean = _predict(muygps, indices, closest_set, test_features, train_features, closest_neighbor, coeffs)
    _sync(test_features)
    time_pred = perf_counter()

    timing = {
        "precompute": time_precomp - time_start,
        "agree": time_agree - time_precomp,
        "nn": time_nn - time_agree,
        "pred": time_pred - time_nn,
    }
    return posterior_mean, coeffs, timing
