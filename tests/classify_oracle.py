"""A numpy statement of the classification path, written from its definitions: the reference's numpy-backend
cross-entropy (_src/optimize/loss/numpy.py:12-19 -- scipy ``softmax`` followed by sklearn's
``log_loss(normalize=False)``, which clips the probabilities to [eps, 1 - eps] with eps the machine epsilon of their
dtype), its cotangent, and the label-agreement rule of ``classify_any`` / ``classify_two_class_uq``
(examples/classify.py:577-591).  A checker only: nothing in the package imports it."""

import numpy as np


def softmax(pred):
    x = np.asarray(pred, dtype=np.float64)
    e = np.exp(x - x.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def _eps(dtype):
    return float(np.finfo(np.dtype(dtype)).eps)


def cross_entropy_rows(pred, target, dtype=np.float64):
    """Per-row ``-sum_c one_hot_c log clip(p_c)``; ``dtype`` names the precision whose epsilon clips."""
    eps = _eps(dtype)
    one_hot = np.asarray(target) > 0.0
    p = np.clip(softmax(pred), eps, 1.0 - eps)
    return -(one_hot * np.log(p)).sum(axis=1)


def cross_entropy(pred, target, dtype=np.float64):
    return float(cross_entropy_rows(pred, target, dtype).sum())


def cross_entropy_grad(pred, target, dtype=np.float64):
    """d cross_entropy / d pred: ``grad_j = sum_{c one-hot, p_c not clipped} (p_j - delta_cj)``."""
    eps = _eps(dtype)
    p = softmax(pred)
    active = (np.asarray(target) > 0.0) & (p >= eps) & (p <= 1.0 - eps)
    return active.sum(axis=1, keepdims=True) * p - active


def mse(pred, target):
    r = np.asarray(pred, dtype=np.float64) - np.asarray(target, dtype=np.float64)
    return float((r * r).sum() / r.size)


def mse_grad(pred, target):
    r = np.asarray(pred, dtype=np.float64) - np.asarray(target, dtype=np.float64)
    return 2.0 * r / r.size


def class_sums(pred, target, dtype=np.float64, huber_delta=1.5):
    """[sum cross-entropy, sum r^2, b R, b, argmax agreements, sum pseudo-Huber(r)]"""
    pred, target = np.asarray(pred, dtype=np.float64), np.asarray(target, dtype=np.float64)
    r = pred - target
    hub = huber_delta**2 * (np.sqrt(1.0 + (r / huber_delta) ** 2) - 1.0)
    agree = (pred.argmax(axis=1) == target.argmax(axis=1)).sum()
    return np.array([cross_entropy(pred, target, dtype), (r * r).sum(), r.size, r.shape[0], agree, hub.sum()])


def partition(labels, nn_indices):
    """(pred (b, R) = first neighbour's labels, nonconstant (b) bool, sel (m) ascending, nn_sel (m, k)): a
    neighbourhood is non-constant iff max != min of label COLUMN 0 over its neighbours -- the reference's rule,
    literally (three or more classes: a neighbourhood mixing classes 1 and 2 counts as constant)."""
    labels, nn_indices = np.asarray(labels), np.asarray(nn_indices)
    col0 = labels[nn_indices, 0]
    nonconstant = col0.max(axis=1) != col0.min(axis=1)
    sel = np.where(nonconstant)[0]
    return labels[nn_indices[:, 0], :], nonconstant, sel, nn_indices[sel]


def near_ties(mean, rtol):
    """Rows whose top two means lie within ``2 rtol (|m| + rms)`` of each other: where an argmax may differ between
    two implementations that agree within ``rtol`` (tests/util.assert_close's bound, on either side)."""
    mean = np.asarray(mean, dtype=np.float64)
    rms = float(np.sqrt(np.mean(mean**2)))
    top = np.sort(mean, axis=1)[:, ::-1]
    return (top[:, 0] - top[:, 1]) <= 2.0 * rtol * (np.abs(top[:, 0]) + rms)


def interval_curves(mean, variance, correct_mask, cutv):
    """alpha / beta of ``train_two_class_interval`` (examples/two_class_classify_uq.py:483-514) on a grid."""
    m1, sd = np.asarray(mean)[:, 1], np.sqrt(np.asarray(variance))
    inside = (m1[None, :] - cutv[:, None] * sd[None, :] < 0.0) & (m1[None, :] + cutv[:, None] * sd[None, :] > 0.0)
    wrong = ~np.asarray(correct_mask)
    return 1.0 - inside[:, wrong].mean(axis=1), inside[:, correct_mask].mean(axis=1)
