"""Launch geometry of the fused_wave_kernel family: every launcher path (built in, run-time shapes, run-time compiled;
forward, coefficients, general Matern, LOOCV, backward) and every branch of the LDS byte sum (csrc/mgp_fused_wave_launch.h:
wave_geometry), one call through the C entry point each, at the smallest shape that takes the path.

What a call reports -- the kernel's name, its workgroups and its dynamic LDS bytes -- is compared with
tests/golden/wave_launch_geometry.json, recorded by this file itself (``python -m tests.test_gpu_wave_launch
--record FILE [--tensors FILE.npz]``) on the build BEFORE the launchers were folded into one geometry function: a
launcher that passes fewer bytes than the kernel lays out reads or writes past its LDS allocation.  Numerical parity
of these paths is the business of the other test files."""

import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wave_launch_geometry.json")
N = 2000  # table rows
JIT_B = 4100  # just past MUYGPYS_HIP_JIT_CACHED_MIN_BATCH (4096): a kernel in the prewarmed cache serves the call

# name: (entry, dtype, k, d, R, b, slots per neighbourhood, options).  b = 5 leaves an odd tail of the two neighbourhoods
# per wave of a 32-slot kernel; the backward launchers take a cached object at any batch size: b = 1.
CASES = {
    "builtin_f32_k30_d40_plain": ("posterior", "float32", 30, 40, 1, 5, 32, {}),
    "builtin_f32_k30_d40_prepared": ("posterior", "float32", 30, 40, 1, 5, 32, {"packed": True}),
    "builtin_f64_k50_d8": ("posterior", "float64", 50, 8, 1, 3, 64, {}),
    "runtime_f32_k12_d8_R2_pipelined": ("posterior", "float32", 12, 8, 2, 5, 32, {}),
    "runtime_f32_k12_d6_staged": ("posterior", "float32", 12, 6, 1, 5, 32, {}),
    "runtime_f64_k20_d8_capped": ("posterior", "float64", 20, 8, 1, 3, 32, {}),
    "runtime_f64_k40_d8": ("posterior", "float64", 40, 8, 1, 3, 64, {}),
    "coefficients_f32_k12_d8": ("fast_coefficients", "float32", 12, 8, 1, 5, 32, {}),
    "gen_f32_k12_d8": ("posterior_gen", "float32", 12, 8, 1, 5, 32, {"smoothness": 1.3}),
    "gen_f64_k12_d8": ("posterior_gen", "float64", 12, 8, 1, 5, 32, {"smoothness": 1.3}),
    "loocv_f32_k30_d40": ("loocv", "float32", 30, 40, 1, 5, 32, {}),
    "jit_f32_k10_d8_prepared": ("posterior", "float32", 10, 8, 1, JIT_B, 16, {"packed": True, "jit": True}),
    "jit_f32_k20_d16_plain_folded": ("posterior", "float32", 20, 16, 1, JIT_B, 32, {"jit": True}),
    "jit_f32_k40_d8_prepared": ("posterior", "float32", 40, 8, 1, JIT_B, 64, {"packed": True, "jit": True}),
    "jit_f64_k40_d8_prepared": ("posterior", "float64", 40, 8, 1, JIT_B, 64, {"packed": True, "jit": True}),
    "backward_f64_k50_d8": ("posterior_backward", "float64", 50, 8, 1, 3, 64, {}),
    "backward_f32_k30_d40": ("posterior_backward", "float32", 30, 40, 1, 5, 32, {}),
    "backward_jit_f64_k40_d8": ("posterior_backward", "float64", 40, 8, 1, 1, 64, {"jit": True}),
    "backward_jit_f32_k30_d16": ("posterior_backward", "float32", 30, 16, 1, 1, 32, {"jit": True}),
    "backward_jit_f32_k50_d8": ("posterior_backward", "float32", 50, 8, 1, 1, 64, {"jit": True}),
    "backward_jit_f32_k30_d100": ("posterior_backward", "float32", 30, 100, 1, 1, 32, {"jit": True}),
}


def run_case(name):
    """One call of the case's C entry point -> (what the library reports of the launch, the call's output tensors)."""
    from muygpys_amd import _lib
    from muygpys_amd.fused import PackedTable

    entry, dtype, k, d, R, b, _, opt = CASES[name]
    td, dev, P = getattr(torch, dtype), torch.device("cuda"), _lib.ptr
    rng = np.random.default_rng(sum(name.encode()))
    X = torch.as_tensor(rng.normal(size=(N, d)), dtype=td, device=dev)
    Y = torch.as_tensor(rng.normal(size=(N, R)), dtype=td, device=dev)
    bi_host = rng.integers(0, N, size=b)
    ni_host = rng.random((b, N - 1)).argsort(axis=1)[:, :k]  # (distinct rows)
    bi = torch.as_tensor(bi_host, device=dev)
    ni = torch.as_tensor(ni_host + (ni_host >= bi_host[:, None]), device=dev)  # (never the query's own row)
    ls = torch.full((1,), 1.2 * float(np.sqrt(d)), dtype=td, device=dev)
    eps = 1e-3 if dtype == "float32" else 1e-5
    kid, mid = _lib.KERNEL_IDS["matern15"], _lib.METRIC_IDS["l2"]
    new = lambda *shape: torch.zeros(shape, dtype=td, device=dev)  # noqa: E731
    info = torch.zeros(1, dtype=torch.int32, device=dev)
    noise = (_lib.NOISE_SCALAR, eps, None)
    out = {}
    if entry == "posterior":
        out = {"mean": new(b, R), "var": new(b), "ykinvy": new(b, R)}
        tail = noise + (kid, mid, P(ls), 1, P(out["mean"]), P(out["var"]), P(out["ykinvy"]), P(info), _lib.stream_ptr())
        if opt.get("packed"):
            t = PackedTable(X, Y)
            rc = _lib.fn("posterior_packed", td)(P(t.data), t.stride, P(t.data), t.stride, d, P(bi), P(ni), b, k, R, *tail)
        else:
            rc = _lib.fn("posterior", td)(P(X), P(X), d, P(bi), P(ni), b, k, P(Y), R, *tail)
    elif entry == "posterior_gen":
        out = {"mean": new(b, R), "var": new(b), "ykinvy": new(b, R)}
        rc = _lib.fn("posterior_gen", td)(P(X), P(X), None, 0, None, 0, d, P(bi), P(ni), b, k, P(Y), R, 0, *noise, opt["smoothness"],
                                          mid, P(ls), 1, P(out["mean"]), P(out["var"]), P(out["ykinvy"]), P(info), _lib.stream_ptr())
    elif entry == "fast_coefficients":
        out = {"coeffs": new(b, k)}
        rc = _lib.fn("fast_coefficients", td)(P(X), d, P(ni), b, k, P(Y), *noise, kid, mid, P(ls), 1, P(out["coeffs"]), P(info),
                                              _lib.stream_ptr())
    elif entry == "loocv":
        out = {"mean": new(b), "var": new(b), "ykinvy": new(b), "partials": torch.zeros(6, dtype=torch.float64, device=dev)}
        rc = _lib.fn("loocv", td)(P(X), d, P(bi), P(ni), b, k, P(Y), *noise, kid, mid, P(ls), 1, P(out["mean"]), P(out["var"]),
                                  P(out["ykinvy"]), P(info), 1.5, P(out["partials"]), P(_lib.loocv_scratch(dev)), _lib.stream_ptr())
    else:  # posterior_backward: the hyper-parameter cotangents only
        gm = torch.as_tensor(rng.normal(size=(b, R)), dtype=td, device=dev)
        gv = torch.as_tensor(rng.normal(size=b), dtype=td, device=dev)
        out = {"grad_ls": new(b, 1), "grad_noise": new(b, k)}
        rc = _lib.fn("posterior_backward", td)(P(X), P(X), d, P(bi), P(ni), b, k, P(Y), R, *noise, kid, mid, P(ls), 1, P(gm), P(gv),
                                               None, None, None, P(out["grad_ls"]), P(out["grad_noise"]), P(info), _lib.stream_ptr())
    _lib.check(rc, f"{name}: mgp_{entry}")
    torch.cuda.synchronize()
    workgroups, lds = _lib.last_launch_geometry()
    seen = {"kernel": _lib.last_kernel(), "workgroups": workgroups, "lds_bytes": lds}
    if entry == "loocv":
        seen["loocv_geometry"] = list(_lib.last_loocv_geometry())
    assert int(info.item()) == 0, f"{name}: {int(info.item())} neighbourhoods were not positive definite"
    return seen, {key: t.cpu().numpy() for key, t in out.items()}


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("name", list(CASES))
def test_launch_geometry_is_the_recorded_one(name, golden):
    from muygpys_amd import _lib

    b, slots, opt = CASES[name][5], CASES[name][6], CASES[name][7]
    if opt.get("jit") and _lib.load().mgp_jit_mode() == 0:
        pytest.skip("MUYGPYS_HIP_JIT=0")
    seen, _ = run_case(name)
    want = golden[name]
    print(name, seen)
    assert seen["kernel"] == want["kernel"]
    assert seen["lds_bytes"] == want["lds_bytes"]
    ntasks = -(-b // (64 // slots))
    if b <= 5:  # (ceil8(ntasks) decides, on any device)
        assert seen["workgroups"] == want["workgroups"] == -(-ntasks // 8) * 8
    else:  # (the device's residency decides)
        assert seen["workgroups"] % 8 == 0 and 8 <= seen["workgroups"] <= -(-ntasks // 8) * 8
    if "loocv_geometry" in want:
        assert seen["loocv_geometry"] == want["loocv_geometry"]


if __name__ == "__main__":
    import argparse

    ap = argparse.ArgumentParser(description="record what every case reports (and, on request, computes)")
    ap.add_argument("--record", required=True, help="JSON file of the reported kernels and geometries")
    ap.add_argument("--tensors", help=".npz file of every output tensor of every case")
    a = ap.parse_args()
    record, tensors = {}, {}
    for case in CASES:
        record[case], outs = run_case(case)
        tensors.update({f"{case}/{key}": v for key, v in outs.items()})
        print(case, record[case], flush=True)
    with open(a.record, "w") as f:
        json.dump(record, f, indent=1, sort_keys=True)
        f.write("\n")
    if a.tensors:
        np.savez(a.tensors, **tensors)
