"""The direct-to-LDS gather of the pipelined wave kernels (csrc/mgp_fused_wave_kernel.h, pipe_issue), every way it can
go wrong at the smallest shape that reaches it: a row in the wrong tile row, a slot written twice or not at all, the query
row fetched with the neighbour table's base or stride, the gather carried across the tasks of a workgroup, the odd tail.

Every output is compared with the fp64 workgroup family on the plain tables (``path="generic", packed=False``) under the
north_star band of tests/util.py; prepared tables against plain tables bit for bit.  Feature 0 of table
row t grows with t (scaled to the length scale, so that it moves the covariances by order one): a neighbour landing in
another neighbour's tile row changes the posterior by order one, not by order 1e-3."""

import numpy as np
import pytest
import torch

from tests.util import RTOL, assert_close

pytestmark = pytest.mark.gpu

N = 2000  # table rows
NQ = 3000  # rows of the separate query table
JIT_B = 4100  # just past MUYGPYS_HIP_JIT_CACHED_MIN_BATCH: the prewarmed cache serves the call

HEADLINE = "mgp::fused_wave_kernel<float,32,30,1,40,true,false,%s,true>"


def _tables(rng, n, d, R):
    X = 0.5 * rng.normal(size=(n, d))
    X[:, 0] = np.arange(n) * (8.0 / n)  # the row number, within about a length scale of its neighbours in the list
    Y = np.sin(X[:, :1] + 0.3 * np.arange(R)[None, :]) + 0.1 * rng.normal(size=(n, R))
    return X, Y


def _neighbours(rng, n, b, k, bi, force_ends=True):
    """k distinct table rows per neighbourhood, never the query's own row; rows 0 and n - 1 in the first lists."""
    ni = rng.random((b, n - 1)).argsort(axis=1)[:, :k]
    ni = ni + (ni >= bi[:, None])
    if force_ends:
        for r in range(min(b, 3)):
            for col, want in ((r % k, 0), ((r + 7) % k, n - 1)):
                if want != bi[r] and want not in ni[r]:
                    ni[r, col] = want
    assert all(len(set(row)) == k for row in ni) and not (ni == bi[:, None]).any()
    return ni


def _spec(d, dtype):
    from muygpys_amd.fused import KernelSpec

    return KernelSpec("matern15", "l2", 1.2 * float(np.sqrt(d)), 1e-3 if dtype == "float32" else 1e-5)


def _run(dtype, d, Xq, Xn, Y, bi, ni, model=None, **kw):
    """``model``: the element type whose nugget the call uses (the fp64 reference takes the nugget of the call it checks)."""
    from muygpys_amd import _lib
    from muygpys_amd.fused import posterior_mean_var

    td, dev = getattr(torch, dtype), torch.device("cuda")
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=td, device=dev)  # noqa: E731
    xn = t(Xn)
    xq = xn if Xq is Xn else t(Xq)
    out = posterior_mean_var(_spec(d, model or dtype), xq, xn, torch.as_tensor(bi, device=dev), torch.as_tensor(ni, device=dev),
                             t(Y), want_ykinvy=True, **kw)
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in out], _lib.last_kernel()


def _check(dtype, d, Xq, Xn, Y, bi, ni, packed, kernel):
    ref, _ = _run("float64", d, Xq, Xn, Y, bi, ni, model=dtype, path="generic", packed=False)
    got, name = _run(dtype, d, Xq, Xn, Y, bi, ni, packed=packed)
    assert name == kernel, name
    for what, g, r in zip(("mean", "var", "ykinvy"), got, ref):
        err = np.abs(g.astype(np.float64) - r)
        print(f"{kernel} packed={packed} b={len(bi)} {what}: max abs err {err.max():.3e}, rms(ref) {np.sqrt(np.mean(r ** 2)):.3e}")
        assert_close(g, r, RTOL[dtype], f"{what}, packed={packed}")
    return got


@pytest.mark.parametrize("b", [1, 2, 3, 45])
def test_headline_shape_rows_land_in_their_tile_rows(b):
    """b = 1: the second half-wave replays the first; 3: odd tail; 45: 23 tasks on 8 workgroups -- a folded pair and an
    unpaired last task, the pipelined gather carried across three tasks of a workgroup."""
    rng = np.random.default_rng(100 + b)
    k, d = 30, 40
    X, Y = _tables(rng, N, d, 1)
    bi = rng.integers(1, N - 1, size=b)
    ni = _neighbours(rng, N, b, k, bi)
    assert 0 in ni and N - 1 in ni
    plain = _check("float32", d, X, X, Y, bi, ni, False, HEADLINE % "false")
    prepared = _check("float32", d, X, X, Y, bi, ni, True, HEADLINE % "true")
    for what, p, q in zip(("mean", "var", "ykinvy"), prepared, plain):
        assert p.tobytes() == q.tobytes(), f"{what}: prepared and plain tables differ"


@pytest.mark.parametrize("packed", [False, True])
def test_headline_shape_query_row_comes_from_the_query_table(packed):
    rng = np.random.default_rng(7)
    k, d, b = 30, 40, 5
    X, Y = _tables(rng, N, d, 1)
    Xq, _ = _tables(rng, NQ, d, 1)
    bi = np.concatenate([[NQ - 1, 0], rng.integers(N, NQ, size=b - 2)])  # (rows the neighbour table does not have)
    ni = _neighbours(rng, N, b, k, np.full(b, -1))
    _check("float32", d, Xq, X, Y, bi, ni, packed, HEADLINE % ("true" if packed else "false"))


JIT_CASES = {
    "f32_k10_d8_prepared": ("float32", 10, 8, True, "mgp::fused_wave_kernel<float,16,10,1,8,true,false,true,true> [run-time compiled]"),
    "f32_k20_d16_plain": ("float32", 20, 16, False, "mgp::fused_wave_kernel<float,32,20,1,16,true,false,false,true> [run-time compiled]"),
    "f32_k40_d8_prepared": ("float32", 40, 8, True, "mgp::fused_wave_kernel<float,64,40,1,8,true,false,true,true> [run-time compiled]"),
    "f64_k40_d8_prepared": ("float64", 40, 8, True, "mgp::fused_wave_kernel<double,64,40,1,8,true,false,true,false> [run-time compiled]"),
}


@pytest.mark.parametrize("name", list(JIT_CASES))
def test_every_other_row_length(name):
    """16, 32 and 64 slots, four / two / one neighbourhood per wave, 3- and 5-slot rows, the static gather that stops
    after the query row, fp64: the run-time compiled shapes of the prewarmed cache."""
    from muygpys_amd import _lib

    if _lib.load().mgp_jit_mode() == 0:
        pytest.skip("MUYGPYS_HIP_JIT=0")
    dtype, k, d, packed, kernel = JIT_CASES[name]
    rng = np.random.default_rng(sum(name.encode()))
    X, Y = _tables(rng, N, d, 1)
    bi = rng.integers(0, N, size=JIT_B)
    ni = _neighbours(rng, N, JIT_B, k, bi)
    _check(dtype, d, X, X, Y, bi, ni, packed, kernel)


def test_built_in_fp64_shape():
    rng = np.random.default_rng(11)
    k, d, b = 50, 8, 3
    X, Y = _tables(rng, N, d, 1)
    bi = rng.integers(0, N, size=b)
    _check("float64", d, X, X, Y, bi, _neighbours(rng, N, b, k, bi), False, "mgp::fused_wave_kernel<double,64,50,1,8,true,false,false,false>")


def test_run_time_shape_kernel_two_responses():
    rng = np.random.default_rng(12)
    k, d, b = 12, 8, 5
    X, Y = _tables(rng, N, d, 2)
    bi = rng.integers(0, N, size=b)
    _check("float32", d, X, X, Y, bi, _neighbours(rng, N, b, k, bi), False, "mgp::fused_wave_kernel<float,32,0,0,0,true,false,false,true>")


def _c_call(entry, dtype, X, Y, bi, ni, k, d, extra=None):
    """One call of a C entry point on the plain tables, as tests/test_gpu_wave_launch.py makes it."""
    from muygpys_amd import _lib

    td, dev, P = getattr(torch, dtype), torch.device("cuda"), _lib.ptr
    b = len(bi)
    x = torch.as_tensor(X, dtype=td, device=dev)
    y = torch.as_tensor(Y, dtype=td, device=dev)
    bi_d, ni_d = torch.as_tensor(bi, device=dev), torch.as_tensor(ni, device=dev)
    ls = torch.full((1,), 1.2 * float(np.sqrt(d)), dtype=td, device=dev)
    noise = (_lib.NOISE_SCALAR, 1e-3, None)  # (the same model in either precision)
    kid, mid = _lib.KERNEL_IDS["matern15"], _lib.METRIC_IDS["l2"]
    new = lambda *shape: torch.zeros(shape, dtype=td, device=dev)  # noqa: E731
    info = torch.zeros(1, dtype=torch.int32, device=dev)
    if entry == "loocv":
        out = {"mean": new(b), "var": new(b), "ykinvy": new(b), "partials": torch.zeros(6, dtype=torch.float64, device=dev)}
        rc = _lib.fn("loocv", td)(P(x), d, P(bi_d), P(ni_d), b, k, P(y), *noise, kid, mid, P(ls), 1, P(out["mean"]), P(out["var"]),
                                  P(out["ykinvy"]), P(info), 1.5, P(out["partials"]), P(_lib.loocv_scratch(dev)), _lib.stream_ptr())
    else:
        gm, gv = (torch.as_tensor(a, dtype=td, device=dev) for a in extra)
        out = {"grad_ls": new(b, 1), "grad_noise": new(b, k)}
        rc = _lib.fn("posterior_backward", td)(P(x), P(x), d, P(bi_d), P(ni_d), b, k, P(y), 1, *noise, kid, mid, P(ls), 1, P(gm), P(gv),
                                               None, None, None, P(out["grad_ls"]), P(out["grad_noise"]), P(info), _lib.stream_ptr())
    _lib.check(rc, f"mgp_{entry}")
    torch.cuda.synchronize()
    assert int(info.item()) == 0
    return {key: t.cpu().numpy() for key, t in out.items()}, _lib.last_kernel()


def test_loocv_entry_headline_shape():
    rng = np.random.default_rng(13)
    k, d, b = 30, 40, 5
    X, Y = _tables(rng, N, d, 1)
    bi = rng.integers(0, N, size=b)
    ni = _neighbours(rng, N, b, k, bi)
    ref, _ = _run("float64", d, X, X, Y, bi, ni, model="float32", path="generic", packed=False)
    got, kernel = _c_call("loocv", "float32", X, Y, bi, ni, k, d)
    assert kernel == HEADLINE % "false", kernel
    for what, r in zip(("mean", "var"), ref):
        print(f"loocv {what}: max abs err {np.abs(got[what] - r.reshape(-1)).max():.3e}")
        assert_close(got[what], r.reshape(-1), RTOL["float32"], what)


def test_backward_headline_shape_against_its_fp64_instantiation():
    """Hyper-parameter cotangents, fp32 against the fp64 instantiation of the same kernel at 3 x rtol (the gradient band)."""
    from muygpys_amd import _lib

    if _lib.load().mgp_jit_mode() == 0:
        pytest.skip("MUYGPYS_HIP_JIT=0")  # (the fp64 instantiation of this shape is a run-time compiled one)
    rng = np.random.default_rng(14)
    k, d, b = 30, 40, 5
    X, Y = _tables(rng, N, d, 1)
    bi = rng.integers(0, N, size=b)
    ni = _neighbours(rng, N, b, k, bi)
    cot = (rng.normal(size=(b, 1)), rng.normal(size=b))
    got, kernel = _c_call("posterior_backward", "float32", X, Y, bi, ni, k, d, cot)
    assert kernel == "mgp::fused_wave_kernel<float,32,30,1,40,true,false,false,true,false,backward>", kernel
    ref, kernel64 = _c_call("posterior_backward", "float64", X, Y, bi, ni, k, d, cot)
    assert "fused_wave_kernel<double,32,30,1,40" in kernel64 and "backward" in kernel64, kernel64
    for what in ("grad_ls", "grad_noise"):
        print(f"backward {what}: max abs err {np.abs(got[what] - ref[what]).max():.3e}, rms(ref) {np.sqrt(np.mean(ref[what] ** 2)):.3e}")
        assert_close(got[what], ref[what], 3 * RTOL["float32"], what)
