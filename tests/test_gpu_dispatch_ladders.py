"""GPU: the last rungs of the fallback ladders launch what the entry named directly launches.

At the edge between the LDS workgroup kernel and the slab kernel (``mgp_max_nn_count``), ``path="auto"`` must end on the
same kernel, on the same inputs, as the family named by ``path=`` -- so the outputs agree bit for bit -- and ``_solve``
on materialised systems must agree bit for bit with a direct ``mgp_solve_large_*`` call.  (Which entries are tried in
which order, and with which arguments: tests/test_dispatch_ladders_cpu.py, without a device.)

b = 5, d = 3; uniform [0, 1]^d points, length scale 0.5, nugget 1e-2, as in tests/test_gpu_large.py."""

import numpy as np
import pytest
import torch

from muygpys_amd import _lib, fused
from muygpys_amd._src.gp.muygps import hip as M
from muygpys_amd.fused import KernelSpec

pytestmark = pytest.mark.gpu

B, D, N = 5, 3, 400
DTYPES = [torch.float32, torch.float64]
SPEC = KernelSpec("matern15", "l2", 0.5, 1e-2)


def kmax(dtype):
    """The last nn_count the LDS-resident kernels serve with one response."""
    return _lib.load().mgp_max_nn_count(dtype.itemsize, 1)


def problem(k, dtype, seed):
    rng = np.random.default_rng(seed)
    X = rng.uniform(size=(N, D))
    y = np.sin(3.0 * X.sum(1)) + 0.1 * rng.normal(size=N)
    bi = rng.choice(N, size=B, replace=False)
    ni = np.stack([rng.choice(N, size=k, replace=False) for _ in range(B)])
    return (torch.tensor(X, device="cuda", dtype=dtype), torch.tensor(y, device="cuda", dtype=dtype),
            torch.tensor(bi, device="cuda"), torch.tensor(ni, device="cuda"))


def by_path(k, dtype, path):
    X, y, bi, ni = problem(k, dtype, seed=k)
    mean, var = fused.posterior_mean_var(SPEC, X, X, bi, ni, y, path=path)
    kernel = _lib.last_kernel()
    torch.cuda.synchronize()
    assert torch.isfinite(mean).all() and torch.isfinite(var).all()
    return mean, var, kernel


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("k_from_limit, named", [(1, "large"), (0, "generic")])
def test_auto_ends_on_the_kernel_the_named_family_launches(dtype, k_from_limit, named):
    k = kmax(dtype) + k_from_limit
    mean, var, kernel = by_path(k, dtype, "auto")
    mean_named, var_named, kernel_named = by_path(k, dtype, named)
    assert kernel == kernel_named and kernel
    assert torch.equal(mean, mean_named) and torch.equal(var, var_named)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_solve_beyond_lds_is_the_direct_slab_call(dtype):
    """Sixteen response columns: ``mgp_solve_*`` keeps no feature tile in LDS, so with one response it still fits
    ``mgp_max_nn_count(es, 1) + 1`` rows there (up to 13 responses in fp32, 11 in fp64, by the LDS arithmetic of
    csrc/mgp_generic.hip); with sixteen it refuses -- asserted below -- and ``_solve`` ends on its slab rung."""
    b, R = 3, 16
    k = kmax(dtype) + 1
    gen = torch.Generator(device="cuda").manual_seed(k)
    P = torch.rand(b, k + 1, D, device="cuda", generator=gen, dtype=torch.float64)
    cov = torch.exp(-torch.cdist(P, P) ** 2 / (2 * 0.5**2))                        # RBF, length scale 0.5
    Kin = (cov[:, :k, :k] + 1e-2 * torch.eye(k, device="cuda", dtype=torch.float64)).to(dtype).contiguous()
    Kcross = cov[:, :k, k].to(dtype).contiguous()
    Y = torch.rand(b, k, R, device="cuda", generator=gen, dtype=torch.float64).to(dtype)
    want = ("mean", "var", "ykinvy", "coeffs")
    got = M._solve(Kin, Kcross, Y, kout=1.0, want=want)
    direct = (torch.empty((b, R), device="cuda", dtype=dtype), torch.empty(b, device="cuda", dtype=dtype),
              torch.empty((b, R), device="cuda", dtype=dtype), torch.empty((b, k, R), device="cuda", dtype=dtype))
    info = torch.zeros(1, device="cuda", dtype=torch.int32)
    ws = torch.empty(_lib.load().mgp_large_workspace_bytes(dtype.itemsize, k, R, b), dtype=torch.uint8, device="cuda")
    assert ws.numel() > 0
    rc = _lib.fn("solve_large", dtype)(_lib.ptr(Kin), _lib.ptr(Kcross), _lib.ptr(Y), b, k, R, 1.0, *map(_lib.ptr, direct),
                                       _lib.ptr(info), _lib.ptr(ws), ws.numel(), _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0 and int(info.item()) == 0
    # (the LDS entry refuses this k: what _solve returned came from its slab rung)
    assert _lib.fn("solve", dtype)(_lib.ptr(Kin), _lib.ptr(Kcross), _lib.ptr(Y), b, k, R, 1.0, *map(_lib.ptr, direct),
                                   _lib.ptr(info), _lib.stream_ptr()) == _lib.EUNSUPPORTED
    for name, a, c in zip(want, got, direct):
        assert torch.isfinite(a).all(), name
        assert torch.equal(a, c), name
