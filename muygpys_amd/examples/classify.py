"""Classification prediction on the hip backend.

Mirrors the prediction half of the reference's ``MuyGPyS.examples.classify`` and
``MuyGPyS.examples.two_class_classify_uq`` -- ``classify_any`` (examples/classify.py:537-607),
``classify_two_class_uq``, ``train_two_class_interval``, ``make_masks`` and ``do_uq``
(examples/two_class_classify_uq.py:251-524) -- with the reference's signatures over device tensors and
:class:`muygpys_amd.neighbors.NN_Wrapper`.  ``make_classifier`` / ``do_classify`` and the deprecated
``MultivariateMuyGPS`` container are not mirrored.

Both classifiers skip the GP solve for test points whose neighbours all carry one label: the nearest
neighbour's label row is the prediction there.  On the device that is k-NN -> ``mgp_class_partition_*`` (label
agreement, the compacted list of the neighbourhoods that still need the solve) -> ONE host read of their number
``m`` -> the fused posterior on those ``m`` rows only -> ``mgp_class_scatter_*``.

The agreement rule is the reference's, literally: a neighbourhood is non-constant iff max != min of label
COLUMN 0 over its neighbours.  With three or more classes a neighbourhood that mixes classes 1 and 2 therefore
counts as constant and takes its nearest neighbour's label.
"""

from __future__ import annotations

from time import perf_counter
from typing import Callable, Dict, List, Tuple, Union

import torch

from muygpys_amd import _lib
from muygpys_amd.neighbors import NN_Wrapper

example_lambdas = [
    lambda alpha, beta, correct_count, incorrect_count: torch.argmin(alpha + beta),
    lambda alpha, beta, correct_count, incorrect_count: torch.argmin(2 * alpha + beta),
    lambda alpha, beta, correct_count, incorrect_count: torch.argmin(4 * alpha + beta),
    lambda alpha, beta, correct_count, incorrect_count: torch.argmin(10 * alpha + beta),
    lambda alpha, beta, correct_count, incorrect_count: torch.argmin(incorrect_count * alpha + correct_count * beta),
]


def _regress_from_indices(surrogate, indices, nn_indices, test_features, train_features, train_labels, want_variance):
    """examples/from_indices.py:42-90 on lazy handles: the mean (and variance) of one fused launch."""
    cross, pair, nn_targets = surrogate.make_predict_tensors(indices, nn_indices, test_features, train_features, train_labels)
    Kin, Kcross = surrogate.kernel(pair), surrogate.kernel(cross)
    mean = surrogate.posterior_mean(Kin, Kcross, nn_targets)
    return mean, (surrogate.posterior_variance(Kin, Kcross) if want_variance else None)


def _partition_and_solve(surrogate, test_features, train_features, nbrs_lookup, train_labels, want_variance,
                         partition: bool = True):
    _lib.require_cuda(test_features, train_features, train_labels)
    labels = train_labels.contiguous()
    if labels.ndim != 2:
        raise ValueError("train_labels must be a one-hot encoding of shape (train_count, class_count)")
    time_start = perf_counter()
    nn_indices, _ = nbrs_lookup.get_nns(test_features)
    nn_indices = nn_indices.to(torch.int64).contiguous()
    time_nn = perf_counter()  # (host time: the device is waited for once, at the read of m -- it falls under "agree")
    b, class_count = nn_indices.shape[0], labels.shape[1]
    pred, nonconstant, count, sel, nn_sel = _lib.class_partition(labels, nn_indices)
    variances = torch.zeros(b, device=labels.device, dtype=labels.dtype) if want_variance else None
    if partition:
        m = int(count.item())  # the one host read of the path
        sel, nn_sel = sel[:m], nn_sel[:m]
    else:  # every neighbourhood solved (what the agreement shortcut saves; timing comparisons)
        m, sel, nn_sel = b, torch.arange(b, device=labels.device), nn_indices
    time_agree = perf_counter()
    if m > 0:
        mean, var = _regress_from_indices(surrogate, sel, nn_sel, test_features, train_features, labels, want_variance)
        mean = mean.reshape(m, class_count).contiguous()
        if want_variance:
            if var.numel() != m:
                raise ValueError("classify_two_class_uq needs one posterior variance per test point (a scalar scale)")
            var = var.reshape(m).to(mean.dtype).contiguous()
        _lib.class_scatter(mean, var, sel, pred, variances)
    torch.cuda.synchronize()
    time_pred = perf_counter()
    timing = {"nn": time_nn - time_start, "agree": time_agree - time_nn, "pred": time_pred - time_agree}
    return pred, variances, nonconstant, timing


def classify_any(surrogate, test_features: torch.Tensor, train_features: torch.Tensor, train_nbrs_lookup: NN_Wrapper,
                 train_labels: torch.Tensor) -> Tuple[torch.Tensor, Dict[str, float]]:
    """examples/classify.py:537-607: the surrogate regression means ``(test_count, class_count)`` of every test item
    and the timing of the subroutines.  Constant neighbourhoods (see the module docstring for the rule) take their
    nearest neighbour's label row; the fused posterior runs on the others only."""
    pred, _, _, timing = _partition_and_solve(surrogate, test_features, train_features, train_nbrs_lookup, train_labels, False)
    return pred, timing


def classify_two_class_uq(surrogate, test_features: torch.Tensor, train_features: torch.Tensor,
                          train_nbrs_lookup: NN_Wrapper, train_labels: torch.Tensor
                          ) -> Tuple[torch.Tensor, torch.Tensor, Dict[str, float]]:
    """examples/two_class_classify_uq.py:346-423: means ``(test_count, 2)``, posterior variances ``(test_count,)`` --
    zero for constant neighbourhoods, as in the reference -- and the timing of the subroutines."""
    if train_labels.ndim != 2 or train_labels.shape[1] != 2:
        raise ValueError("classify_two_class_uq takes two-column one-hot labels")
    pred, variances, _, timing = _partition_and_solve(surrogate, test_features, train_features, train_nbrs_lookup,
                                                      train_labels, True)
    return pred, variances, timing


def interval_curves(mean: torch.Tensor, variance: torch.Tensor, correct_mask: torch.Tensor, cutv: torch.Tensor):
    """alpha (type-1) and beta (type-2) rates of ``train_two_class_interval`` at every grid value
    (two_class_classify_uq.py:483-514): the share of wrongly / correctly classified batch points whose interval
    ``mean[:, 1] +- cut sqrt(variance)`` contains 0."""
    m1, sd = mean[:, 1], torch.sqrt(variance)
    inside = ((m1[None, :] - cutv[:, None] * sd[None, :]) < 0.0) & ((m1[None, :] + cutv[:, None] * sd[None, :]) > 0.0)
    wrong = ~correct_mask
    alpha = 1.0 - inside[:, wrong].to(mean.dtype).mean(dim=1)
    beta = inside[:, correct_mask].to(mean.dtype).mean(dim=1)
    return alpha, beta


def train_two_class_interval(surrogate, batch_indices: torch.Tensor, batch_nn_indices: torch.Tensor,
                             train_features: torch.Tensor, train_responses: torch.Tensor, train_labels: torch.Tensor,
                             objective_fns: Union[List[Callable], Tuple[Callable, ...]]) -> torch.Tensor:
    """two_class_classify_uq.py:426-524: the confidence-interval scale that minimises each objective, on the
    reference's grid ``linspace(0.01, 20, 1999)`` with ``sqrt(variance)``.  ``train_responses`` is the one-hot
    ``(train_count, 2)`` table, ``train_labels`` the class labels in {-1, 1}; an objective takes ``(alpha, beta,
    correct_count, incorrect_count)`` and returns a grid index (:data:`example_lambdas`)."""
    targets = train_labels[batch_indices]
    mean, variance = _regress_from_indices(surrogate, batch_indices, batch_nn_indices, train_features, train_features,
                                           train_responses, True)
    predicted_labels = 2 * torch.argmax(mean, dim=1) - 1
    correct_mask = predicted_labels == targets
    cutv = torch.linspace(0.01, 20, 1999, device=mean.device, dtype=mean.dtype)
    alpha, beta = interval_curves(mean, variance.reshape(-1), correct_mask, cutv)
    correct_count, incorrect_count = correct_mask.sum(), (~correct_mask).sum()
    return torch.stack([cutv[obj_f(alpha, beta, correct_count, incorrect_count)] for obj_f in objective_fns])


def make_masks(predictions: torch.Tensor, cutoffs: torch.Tensor, variances: torch.Tensor, mid_value: float) -> torch.Tensor:
    """two_class_classify_uq.py:251-291: ``(objective_count, test_count)`` masks of the test points whose interval
    ``predictions[:, 1] +- cut * variances`` contains ``mid_value`` (the reference scales by the variance here, not
    by its root: kept)."""
    v = variances.reshape(predictions.shape[0])
    p1 = predictions[:, 1]
    cut = cutoffs.reshape(-1, 1).to(p1.dtype)
    return ((p1[None, :] - cut * v[None, :]) < mid_value) & ((p1[None, :] + cut * v[None, :]) > mid_value)


def do_uq(surrogate_predictions: torch.Tensor, test_labels: torch.Tensor, masks: torch.Tensor) -> Tuple[float, torch.Tensor]:
    """two_class_classify_uq.py:294-343: overall accuracy and, per mask, (ambiguous count, accuracy of the ambiguous,
    accuracy of the unambiguous); an empty mask reports 0 for its accuracy, an empty complement NaN, as numpy's mean
    of an empty selection does."""
    correct = (torch.argmax(surrogate_predictions, dim=1) == torch.argmax(test_labels, dim=1)).to(torch.float64)
    mk = masks.to(torch.float64)
    inside, outside = mk.sum(dim=1), (1.0 - mk).sum(dim=1)
    acc_in = (mk * correct[None, :]).sum(dim=1) / inside
    acc_out = ((1.0 - mk) * correct[None, :]).sum(dim=1) / outside
    acc_in = torch.where(inside == 0, torch.zeros_like(acc_in), acc_in)
    return float(correct.mean()), torch.stack([inside, acc_in, acc_out], dim=1)
