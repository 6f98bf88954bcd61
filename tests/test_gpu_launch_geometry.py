"""Launch geometry of the workgroup and wave families outside fused_wave_kernel (that family: test_gpu_wave_launch.py):
every launcher path that notes a kernel name, one call through the C entry point each, at the smallest shape that takes
the path, with at most five neighbourhoods.

What a call reports -- the kernel's name, its workgroups and its dynamic LDS bytes -- is compared with
tests/golden/launch_geometry.json, recorded by this file itself (``python -m tests.test_gpu_launch_geometry --record
FILE``) on the build BEFORE the host-side launch rules moved into csrc/mgp_launch.h.  fused_large_kernel,
hyper_backward_large_kernel and posterior_backward_large_kernel noted a name but no geometry on that build: their
entries were recorded from a copy of it with nothing but the missing ``note_launch_geometry(grid, lds)`` line added to
the three launchers.  With so few neighbourhoods the grid is the number of work units on any device (a neighbourhood; a
pair of them under FOLD; a slab of the workspace), so the workgroup count is held to equality.  Numerical parity of these
paths is the business of the other test files; the launchers that note no name share the grid functions checked here."""

import json
import os

import numpy as np
import pytest
import torch

from tests import shear_cases as S

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "launch_geometry.json")
N = 2000  # table rows

# name: (entry, dtype, k, d, R, b, work units, kernel the case is about, options).  k: a number, "k0" (the first
# nn_count the LDS workgroup kernel refuses: mgp_max_nn_count + 1) or "kb" (mgp_max_nn_count_backward(8) + 1), read when
# the test runs.  yk=False: no y^T K^-1 y asked for (prediction); misaligned: tables 4 bytes off a 16-byte boundary.
CASES = {
    # fused_rhs_kernel: four and sixteen response columns, Gram and difference form, the back-substituting variants
    "rhs_f32_R1_d8_gram": ("posterior_rhs", "float32", 20, 8, 1, 5, 5, "fused_rhs_kernel<float,4,false,true>", {}),
    "rhs_f32_R1_d6_diff": ("posterior_rhs", "float32", 20, 6, 1, 5, 5, "fused_rhs_kernel<float,4,false,false>", {}),
    "rhs_f32_R16_d8_gram": ("posterior_rhs", "float32", 20, 8, 16, 5, 5, "fused_rhs_kernel<float,16,false,true>", {}),
    "rhs_f32_R16_d6_diff_back": ("posterior_rhs", "float32", 20, 6, 16, 5, 5, "fused_rhs_kernel<float,16,true,false>", {"yk": False}),
    "rhs_f32_R16_d48_fold": ("posterior_rhs", "float32", 20, 48, 16, 5, 3, "fused_rhs_kernel<float,16,true,true,fold>", {"yk": False}),
    "rhs_f32_R16_d8_w3": ("posterior_rhs", "float32", 20, 8, 16, 5, 5, "fused_rhs_kernel<float,16,true,true,w3>", {"yk": False, "misaligned": True}),
    "rhs_f64_R1_d8": ("posterior_rhs", "float64", 20, 8, 1, 5, 5, "fused_rhs_kernel<double,4,false,false>", {}),
    "rhs_f64_R16_d8_back": ("posterior_rhs", "float64", 20, 8, 16, 5, 5, "fused_rhs_kernel<double,16,true,false>", {"yk": False}),
    "rhs_mf_f32_k20_d8_R16_plain": ("posterior_rhs", "float32", 20, 8, 16, 5, 5, "fused_rhs_mf_kernel<16>", {"yk": False}),
    "rhs_mf_f32_k20_d8_R16_prepared": ("posterior_packed", "float32", 20, 8, 16, 5, 5, "fused_rhs_mf_kernel<16> [prepared tables]", {"yk": False}),
    # the 128-slot kernels: the smallest column-group count and one in the middle (k = 64 is still the rhs-column kernel's)
    "wide_f32_k64_R1": ("posterior", "float32", 64, 8, 1, 5, 5, "fused_rhs_kernel<float,4,false,true>", {}),
    "wide_f32_k65_R1_ng17": ("posterior", "float32", 65, 8, 1, 5, 5, "fused_wide_kernel<17>", {}),
    "wide_f32_k100_R1_ng26": ("posterior", "float32", 100, 8, 1, 5, 5, "fused_wide_kernel<26>", {}),
    "wide64_f64_k66_R1_nb18": ("posterior", "float64", 66, 8, 1, 5, 5, "fused_wide64_kernel<18>", {}),
    "wide64_f64_k100_R1_nb26": ("posterior", "float64", 100, 8, 1, 5, 5, "fused_wide64_kernel<26>", {}),
    # the LDS workgroup kernel: below and above the 64 KiB of dynamic LDS a kernel gets without asking
    "generic_f32_k12_d8": ("posterior_generic", "float32", 12, 8, 1, 5, 5, "fused_generic_kernel<float>", {}),
    "generic_f64_k12_d8": ("posterior_generic", "float64", 12, 8, 1, 5, 5, "fused_generic_kernel<double>", {}),
    "generic_f32_k140_d8_optin": ("posterior_generic", "float32", 140, 8, 1, 5, 5, "fused_generic_kernel<float>", {"above_64k": True}),
    # the slab kernels: one workgroup per slab of the workspace
    "large_f32_k0_one_slab": ("posterior_large", "float32", "k0", 8, 1, 2, 1, "fused_large_kernel<float>", {"slabs": 1}),
    "large_f32_k0_two_slabs": ("posterior_large", "float32", "k0", 8, 1, 2, 2, "fused_large_kernel<float>", {"slabs": 2}),
    "large_f64_k0_one_slab": ("posterior_large", "float64", "k0", 8, 1, 2, 1, "fused_large_kernel<double>", {"slabs": 1}),
    "large_f64_k0_two_slabs": ("posterior_large", "float64", "k0", 8, 1, 2, 2, "fused_large_kernel<double>", {"slabs": 2}),
    "hyper_backward_large_f64": ("hyper_backward_large", "float64", "kb", 8, 1, 2, 2, "hyper_backward_large_kernel<double>", {"slabs": 2}),
    "posterior_backward_large_f64": ("posterior_backward_large", "float64", "kb", 8, 1, 2, 2, "posterior_backward_large_kernel<double>", {"slabs": 2}),
}
# the packed-triangle kernels on either side of a 64 KiB request: the fused posterior at the neighbour counts
# tests/shear_cases.py names (PAIR_64K), the materialised solve with three cross columns and one response at the row
# counts next to them (3 k rows; in fp32 its smaller carve crosses one neighbour later)
SOLVE_64K = {"float64": (117, 120), "float32": (171, 174)}
for _dtype, _t in (("float64", "double"), ("float32", "float")):
    for _i, _above in enumerate((False, True)):
        for _in in (3, 2):
            _k = S.PAIR_64K[_dtype, _in][_i]
            CASES[f"shear_{_dtype}_in{_in}_k{_k}"] = ("shear_posterior", _dtype, _k, 2, _in, 3, 3, f"shear_posterior_kernel<{_t},{_in}>",
                                                      {"above_64k": _above})
        _n = SOLVE_64K[_dtype][_i]
        CASES[f"solve_multi_{_dtype}_n{_n}"] = ("solve_multi", _dtype, _n, 0, 1, 3, 3, f"solve_multi_kernel<{_t}>", {"above_64k": _above})


def _nn_count(k, lib):
    if k == "k0":
        return lambda es: lib.mgp_max_nn_count(es, 1) + 1
    if k == "kb":
        return lambda es: lib.mgp_max_nn_count_backward(es) + 1
    return lambda es: k


def _shear_call(entry, dtype, k, in_count, b):
    from muygpys_amd import _lib

    td, dev, P = getattr(torch, dtype), torch.device("cuda"), _lib.ptr
    info = torch.zeros(1, dtype=torch.int32, device=dev)
    new = lambda *shape: torch.zeros(shape, dtype=td, device=dev)  # noqa: E731
    if entry == "solve_multi":
        s = S.spd_systems(b, k, 3, 1)
        K, Kc, Y = (torch.as_tensor(a, dtype=td, device=dev) for a in (s.K, s.Kc, s.Y))
        rc = _lib.fn("solve_multi", td)(P(K), P(Kc), P(Y), b, k, 3, 1, P(new(b, 3, 1)), P(new(b, 3, 3)), P(new(b, 1)), P(info),
                                        _lib.stream_ptr())
        return rc, info
    prob = S.problem()
    bi_host = np.arange(b, dtype=np.int64)
    bi = torch.as_tensor(bi_host, device=dev)
    ni = torch.as_tensor(np.ascontiguousarray(prob.order[bi_host, :k]).astype(np.int64), device=dev)
    X, FQ = (torch.as_tensor(a, dtype=td, device=dev) for a in (prob.X.copy(), prob.FQ.copy()))
    Y = torch.as_tensor(np.array(prob.Y[:, 3 - in_count:]), dtype=td, device=dev)
    rc = _lib.fn("shear_posterior", td)(P(FQ), P(X), P(bi), P(ni), b, k, in_count, P(Y), in_count, 0, S.LENGTH_SCALE,
                                        _lib.SHEAR_NOISE_HOMOSCEDASTIC, S.NOISE, P(new(b, 3)), P(new(b, 3, 3)), P(new(b)), P(info),
                                        _lib.stream_ptr())
    return rc, info


def run_case(name):
    """One call of the case's C entry point -> what the library reports of the launch."""
    from muygpys_amd import _lib
    from muygpys_amd.fused import PackedTable

    entry, dtype, k, d, R, b, _, _, opt = CASES[name]
    lib = _lib.load()
    td, dev, P = getattr(torch, dtype), torch.device("cuda"), _lib.ptr
    es = 4 if dtype == "float32" else 8
    k = _nn_count(k, lib)(es)
    if entry in ("shear_posterior", "solve_multi"):
        rc, info = _shear_call(entry, dtype, k, R, b)
    else:
        rng = np.random.default_rng(sum(name.encode()))

        def table(a):  # (misaligned: the same rows, 4 bytes off a 16-byte boundary)
            t = torch.as_tensor(a, dtype=td, device=dev)
            if not opt.get("misaligned"):
                return t
            buf = torch.empty(t.numel() + 1, dtype=td, device=dev)  # (an allocation starts on a boundary)
            view = buf[1:].view(t.shape)
            view.copy_(t)
            assert view.data_ptr() % 16 != 0
            return view

        X = table(rng.normal(size=(N, d)))
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
        model = noise + (kid, mid, P(ls), 1)
        yk = new(b, R) if opt.get("yk", True) else None
        outs = (P(new(b, R)), P(new(b)), P(yk), P(info))
        if entry in ("posterior", "posterior_rhs", "posterior_generic"):
            rc = _lib.fn(entry, td)(P(X), P(X), d, P(bi), P(ni), b, k, P(Y), R, *model, *outs, _lib.stream_ptr())
        elif entry == "posterior_packed":
            t = PackedTable(X, Y)
            rc = _lib.fn(entry, td)(P(t.data), t.stride, P(t.data), t.stride, d, P(bi), P(ni), b, k, R, *model, *outs, _lib.stream_ptr())
        elif entry == "posterior_large":
            size = opt["slabs"] * lib.mgp_large_workspace_bytes(es, k, R, 1)
            ws = torch.empty(size, dtype=torch.uint8, device=dev)
            rc = _lib.fn(entry, td)(P(X), P(X), d, P(bi), P(ni), b, k, P(Y), R, 0, *model, *outs, P(ws), size, _lib.stream_ptr())
        else:  # the two backwards on the slab factor
            size = opt["slabs"] * lib.mgp_backward_large_workspace_bytes(es, k, 1)
            ws = torch.empty(size, dtype=torch.uint8, device=dev)
            gm, gv = (torch.as_tensor(rng.normal(size=s), dtype=td, device=dev) for s in ((b, R), (b,)))
            tail = (P(new(b, 1)), P(new(b, k)), P(info), P(ws), size, _lib.stream_ptr())
            if entry == "hyper_backward_large":
                rc = _lib.fn(entry, td)(P(X), d, P(bi), P(ni), b, k, P(Y), R, *model, P(gm), P(gv), None, *tail)
            else:
                rc = _lib.fn(entry, td)(P(X), P(X), d, P(bi), P(ni), b, k, P(Y), R, *model, P(gm), P(gv), None, None, None, *tail)
    _lib.check(rc, f"{name}: mgp_{entry}")
    torch.cuda.synchronize()
    workgroups, lds = _lib.last_launch_geometry()
    assert int(info.item()) == 0, f"{name}: {int(info.item())} systems were not positive definite"
    return {"kernel": _lib.last_kernel(), "workgroups": workgroups, "lds_bytes": lds}


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("name", list(CASES))
def test_launch_geometry_is_the_recorded_one(name, golden):
    units, kernel, opt = CASES[name][6], CASES[name][7], CASES[name][8]
    seen = run_case(name)
    want = golden[name]
    print(name, seen)
    assert seen["kernel"] == want["kernel"] == "mgp::" + kernel
    assert seen["lds_bytes"] == want["lds_bytes"]
    assert seen["workgroups"] == want["workgroups"] == units
    if "above_64k" in opt:  # (above: the launch depends on the dynamic-LDS attribute)
        assert (seen["lds_bytes"] > 64 * 1024) == opt["above_64k"]


if __name__ == "__main__":
    import argparse

    ap = argparse.ArgumentParser(description="record what every case reports")
    ap.add_argument("--record", required=True, help="JSON file of the reported kernels and geometries")
    a = ap.parse_args()
    record = {}
    for case in CASES:
        record[case] = run_case(case)
        print(case, record[case], flush=True)
    with open(a.record, "w") as f:
        json.dump(record, f, indent=1, sort_keys=True)
        f.write("\n")
