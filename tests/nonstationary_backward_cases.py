"""Hyper-parameter backward with a length scale per neighbourhood (mgp_hyper_backward_ns_*, mgp_hyper_backward_ns_large_*;
fused.loocv_value_and_grad with KernelSpec.length_scale_batch): the cases of tests/test_gpu_nonstationary_backward.py and
a plain fp64 reference -- for every neighbourhood the dense posterior written in torch on the CPU, its scales a leaf
that requires grad, the cotangents contracted and ``autograd.grad`` taken: the rows of g_l (b, ls_count) and g_n (b, k).

The inputs are those of tests/nonstationary_cases.py (``problem``, ``draw_scales``: scales log-uniform over [0.2, 5]
across the batch) on ONE table: the query of neighbourhood nb is training row bi[nb], as in LOOCV.  A query that is one
of its own neighbours is at distance zero of it; under l2 the kernels give such a pair no distance gradient, and the
reference takes the same subgradient (the root is masked, not differentiated, at zero)."""

import functools

import numpy as np
import torch

from tests import nonstationary_cases as NC

B = 7
RUNGS = ("wave", "lds", "slab")


def backward_max(dtype):
    from muygpys_amd import _lib

    return int(_lib.load().mgp_max_nn_count_backward(NC.ES[dtype]))


def case(rung, dtype, k, d, *, aniso=False, kernel="matern15", metric="l2", b=B, noise="scalar"):
    """A case of nonstationary_cases (registered there, so that ``NC.problem`` draws its inputs) with the rung that must
    serve it: "wave" / "lds" through mgp_hyper_backward_ns_*, "slab" through mgp_hyper_backward_ns_large_*."""
    k = backward_max(dtype) + 3 if k == "max+3" else k
    c = NC._case("bwd-" + rung, dtype, k, d, R=3, aniso=aniso, kernel=kernel, metric=metric, b=b, noise=noise)
    c["rung"] = rung
    return NC.BY_ID.setdefault(c["id"], c)


def _reference_cases():
    out = []
    for dt in ("float32", "float64"):
        # (wave: the smallest slot count with an odd tail and unaligned rows; two per wave; one per wave)
        out += [case("wave", dt, 5, 3, noise="table"), case("wave", dt, 20, 8, kernel="rbf", metric="F2"), case("wave", dt, 40, 8),
                case("lds", dt, 10, 12, aniso=True, noise="table"), case("lds", dt, 70, 8, kernel="rbf", metric="F2"),
                case("slab", dt, 40, 8, aniso=True, noise="table"), case("slab", dt, "max+3", 8, b=3)]
    return out


REFERENCE_CASES = _reference_cases()


def cotangents(case_id, b):
    """(gm (b, 3), gv (b,), gyk (b,)) of O(1), fixed per case."""
    rng = np.random.default_rng([NC.SEED, 77, len(case_id)])
    return rng.normal(size=(b, 3)), rng.normal(size=b), rng.normal(size=b)


def kappa(kernel, metric, acc):
    """The covariance of a pair at the summed squares ``acc`` of its scaled differences (torch, differentiable)."""
    if metric == "F2":
        x = acc
    else:
        pos = acc > 0
        x = torch.sqrt(torch.where(pos, acc, torch.ones_like(acc))) * pos
    if kernel == "rbf":
        return torch.exp(-x / 2.0)
    assert kernel == "matern15"
    return (1.0 + np.sqrt(3.0) * x) * torch.exp(-np.sqrt(3.0) * x)


def dense_posterior(kernel, metric, X, bi, ni, Y, ls, eps):
    """(mean (b, R), var (b,), ykinvy (b, R)) of every neighbourhood, dense, torch fp64 on the CPU: ``ls`` (b, 1) or
    (b, d) and ``eps`` (b, k) may require grad."""
    pts = torch.cat([X[ni], X[bi][:, None, :]], dim=1) / ls[:, None, :]   # (b, k + 1, d), scaled
    acc = ((pts[:, :, None, :] - pts[:, None, :, :]) ** 2).sum(-1)
    K = kappa(kernel, metric, acc)
    k = ni.shape[1]
    Kin = K[:, :k, :k] + torch.diag_embed(eps)
    c = K[:, :k, k]
    Yn = Y[ni]                                                             # (b, k, R)
    sol = torch.linalg.solve(Kin, torch.cat([c[:, :, None], Yn], dim=2))
    mean = torch.einsum("bk,bkr->br", c, sol[:, :, 1:])
    var = 1.0 - torch.einsum("bk,bk->b", c, sol[:, :, 0])
    yk = torch.einsum("bkr,bkr->br", Yn, sol[:, :, 1:])
    return mean, var, yk


@functools.lru_cache(maxsize=None)
def reference(case_id, loocv):
    """(g_l (b, ls_count), g_n (b, k)) in fp64, read-only.  ``loocv``: the form with gyk on the first response column
    (R = 1: gm's first column), else the posterior form on all three columns (no y^T K^-1 y)."""
    c, P = NC.BY_ID[case_id], NC.problem(case_id)
    gm, gv, gyk = (torch.tensor(g) for g in cotangents(case_id, P.b))
    ls = torch.tensor(np.array(P.ls), requires_grad=True)
    eps = torch.tensor(np.array(P.noise_rows), requires_grad=True)
    Y = torch.tensor(P.Y[:, :1] if loocv else P.Y)
    mean, var, yk = dense_posterior(c["kernel"], c["metric"], torch.tensor(P.Xn), torch.tensor(P.bi), torch.tensor(P.ni), Y, ls, eps)
    loss = (gv * var).sum() + ((gm[:, :1] * mean).sum() + (gyk * yk[:, 0]).sum() if loocv else (gm * mean).sum())
    out = tuple(g.numpy() for g in torch.autograd.grad(loss, [ls, eps]))
    for a in out:
        a.setflags(write=False)
    return out
