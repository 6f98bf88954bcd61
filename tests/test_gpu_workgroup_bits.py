"""Bits of the LDS and slab workgroup kernels (csrc/mgp_generic.hip, mgp_large.hip, mgp_backward.hip,
mgp_backward_large.hip, mgp_backward_large_full.hip): every case is one call through the C entry that names the family,
9 neighbourhoods over a 600-row table, and what it returns is compared BYTE FOR BYTE with tests/golden/workgroup_bits.json.

The file records its own golden (``python -m tests.test_gpu_workgroup_bits --record FILE``); the committed one was
recorded on the build BEFORE the front end of these kernels -- index list, chunked gather, pair loop, covariance, nugget,
responses, the cotangent pieces -- moved into csrc/mgp_assemble.h and the two output routines became one emit_outputs,
twice, and the two recordings were identical.  The kernels' sums run in a fixed order (one wave's butterfly;
block_sum_ordered; backward_large_ls_chunk), so a neighbourhood's bits depend on nothing but its own inputs: a byte that
differs is a change of arithmetic, never noise.

Compared: mean, variance and y^T K^-1 y of every forward case, the coefficients of the two materialised solves,
grad_noise of every backward case and grad_ls of the two slab backwards.  Not compared (they leave through
floating-point atomics and stay with the tolerance tests of test_gpu_backward.py / test_gpu_large_full_backward.py): the
feature and response cotangents, and grad_ls of the LDS backward_kernel.

Two notes on the entries.  mgp_posterior_generic_* has no gathered-response argument, so its (12, 3, 3) shape runs with
``batch_idx == NULL`` on the table responses there, and with gathered responses AND ``batch_idx == NULL`` through
mgp_posterior_gen_generic_*, the entry of the same kernel body that has the argument.  The LDS backward_kernel is reached
at k = 70, d = 70 whatever MGP_BACKWARD_DLT says (k + 2 > 64 and d > 64 are beyond both wave-sized backwards, which every
such case asserts through mgp_jit_prepare_backward); the library reads that variable once per process, so only the
recording process sets it."""

import base64
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "workgroup_bits.json")
N, B = 600, 9  # table rows, neighbourhoods
NU = 1.7       # the general smoothness: not a half-integer

# name -> (entry, k, R, d, options).  Options: noise "scalar" | "table" | "batch"; aniso; gathered; no_bi (batch_idx NULL);
# kernel / metric (matern15 / l2 unless named); form "loocv" (grad_ykinvy given, R = 1) | "posterior"; sweep (the
# accumulated cotangents are asked for too, into buffers nobody compares); no_grad_ls (grad_ls NULL).  Every case runs in
# both dtypes.
CASES = {}
for _noise in ("scalar", "table", "batch"):
    _model = {"kernel": "rbf", "metric": "F2"} if _noise == "table" else {}  # (F2 under Isotropy: 1 / l^2)
    CASES[f"generic_k12_R3_d3_{_noise}"] = ("posterior_generic", 12, 3, 3, {"noise": _noise, **_model})
CASES["generic_k12_R3_d3_no_bi"] = ("posterior_generic", 12, 3, 3, {"no_bi": True})
CASES["gen_generic_k12_R3_d3_gathered_no_bi"] = ("posterior_gen_generic", 12, 3, 3, {"gathered": True, "no_bi": True})
CASES["generic_k70_R1_d70_iso"] = ("posterior_generic", 70, 1, 70, {})
CASES["generic_k70_R1_d70_aniso"] = ("posterior_generic", 70, 1, 70, {"aniso": True, "kernel": "rbf", "metric": "F2"})
CASES["generic_k65_R3_d72"] = ("posterior_generic", 65, 3, 72, {"noise": "table"})
CASES["gen_generic_k70_R1_d8"] = ("posterior_gen_generic", 70, 1, 8, {})
CASES["large_k33_R2_d5"] = ("posterior_large", 33, 2, 5, {"noise": "table", "gathered": True, "kernel": "rbf", "metric": "F2"})
CASES["large_k130_R1_d72"] = ("posterior_large", 130, 1, 72, {"noise": "batch", "aniso": True})
CASES["gen_large_k33_R1_d8"] = ("posterior_gen_large", 33, 1, 8, {})
CASES["solve_generic_k12_R2"] = ("solve", 12, 2, 0, {})
CASES["solve_large_k33_R2"] = ("solve_large", 33, 2, 0, {})
for _k in (33, 130):
    for _d in (5, 72):
        for _aniso in (False, True):
            _tag = f"k{_k}_d{_d}_{'aniso' if _aniso else 'iso'}"
            _noise = {(33, 5): "scalar", (33, 72): "table", (130, 5): "batch", (130, 72): "scalar"}[_k, _d]
            _model = {"kernel": "rbf", "metric": "F2"} if _d == 5 else {}
            CASES[f"hyper_backward_large_{_tag}"] = ("hyper_backward_large", _k, 1 if _d == 5 else 2, _d,
                                                     {"noise": _noise, "aniso": _aniso, "form": "loocv" if _d == 5 else "posterior", **_model})
            CASES[f"posterior_backward_large_{_tag}"] = ("posterior_backward_large", _k, 2, _d,
                                                         {"noise": _noise, "aniso": _aniso, "sweep": _d == 72, **_model})
# (grad_noise alone, the features in one chunk: the slab assembly keeps no distances)
CASES["hyper_backward_large_k33_d5_noise_only"] = ("hyper_backward_large", 33, 1, 5, {"noise": "table", "form": "loocv", "no_grad_ls": True})
for _noise in ("scalar", "table", "batch"):
    CASES[f"backward_k70_R2_d70_{_noise}"] = ("posterior_backward", 70, 2, 70, {"noise": _noise, "aniso": _noise == "table"})
CASES["loocv_backward_k70_d70"] = ("loocv_backward", 70, 1, 70, {"kernel": "rbf", "metric": "F2"})
DTYPES = ("float32", "float64")


def _solve_case(entry, td, k, R, rng):
    from muygpys_amd import _lib

    dev, P = torch.device("cuda"), _lib.ptr
    A = rng.normal(size=(B, k, k))
    K = torch.as_tensor(A @ A.transpose(0, 2, 1) / k + np.eye(k), dtype=td, device=dev)
    Kc, Y = (torch.as_tensor(rng.normal(size=s), dtype=td, device=dev) for s in ((B, k), (B, k, R)))
    new = lambda *shape: torch.zeros(shape, dtype=td, device=dev)  # noqa: E731
    out = {"mean": new(B, R), "var": new(B), "ykinvy": new(B, R), "coeffs": new(B, k, R)}
    info = torch.zeros(1, dtype=torch.int32, device=dev)
    args = (P(K), P(Kc), P(Y), B, k, R, 1.25, *(P(out[n]) for n in ("mean", "var", "ykinvy", "coeffs")), P(info))
    if entry == "solve_large":
        size = 2 * _lib.load().mgp_large_workspace_bytes(K.element_size(), k, R, 1)
        ws = torch.empty(size, dtype=torch.uint8, device=dev)
        rc = _lib.fn(entry, td)(*args, P(ws), size, _lib.stream_ptr())
    else:
        rc = _lib.fn(entry, td)(*args, _lib.stream_ptr())
    return rc, info, out


def run_case(name, dtype):
    """One call of the case's C entry -> {output name: bytes}."""
    from muygpys_amd import _lib

    entry, k, R, d, opt = CASES[name]
    lib = _lib.load()
    td, dev, P = getattr(torch, dtype), torch.device("cuda"), _lib.ptr
    es = 4 if dtype == "float32" else 8
    rng = np.random.default_rng(sum(name.encode()))
    if entry in ("solve", "solve_large"):
        rc, info, out = _solve_case(entry, td, k, R, rng)
    else:
        to = lambda a: torch.as_tensor(a, dtype=td, device=dev)  # noqa: E731
        new = lambda *shape: torch.zeros(shape, dtype=td, device=dev)  # noqa: E731
        Xn, Xq, Y = to(rng.normal(size=(N, d))), to(rng.normal(size=(N, d))), to(rng.normal(size=(N, R)))
        one_table = entry in ("hyper_backward_large", "loocv_backward")
        if one_table:
            Xq = Xn
        bi_host = np.arange(B) if opt.get("no_bi") else rng.choice(N, size=B, replace=False)
        ni_host = rng.random((B, N - 1)).argsort(axis=1)[:, :k]  # (distinct rows)
        ni_host = ni_host + (ni_host >= bi_host[:, None])        # (never the query's own row)
        bi = None if opt.get("no_bi") else torch.as_tensor(bi_host, device=dev)
        ni = torch.as_tensor(ni_host, device=dev)
        tg = Y[ni].contiguous() if opt.get("gathered") else Y
        # well-conditioned systems in either precision: off-diagonal covariances of a few per cent
        scale = 0.5 * float(np.sqrt(d))
        ls = to(scale * (0.8 + 0.4 * rng.random(d))) if opt.get("aniso") else to([scale])
        eps = 1e-2 if dtype == "float32" else 1e-4
        nz_table, nz_batch = to(eps * (1.0 + rng.random(N))), to(eps * (1.0 + rng.random((B, k))))
        noise = {"scalar": (_lib.NOISE_SCALAR, eps, None), "table": (_lib.NOISE_TABLE, 0.0, P(nz_table)),
                 "batch": (_lib.NOISE_BATCH, 0.0, P(nz_batch))}[opt.get("noise", "scalar")]
        mid = _lib.METRIC_IDS[opt.get("metric", "l2")]
        kid = _lib.KERNEL_IDS[opt.get("kernel", "matern15")]
        gen = entry.startswith("posterior_gen_")
        model = noise + ((NU,) if gen else (kid,)) + (mid, P(ls), ls.numel())
        info = torch.zeros(1, dtype=torch.int32, device=dev)
        head = (P(Xq), P(Xn), d, P(bi), P(ni), B, k, P(tg), R)
        if entry.startswith("posterior_large") or gen:
            head += (int(bool(opt.get("gathered"))),)
        if entry in ("posterior_generic", "posterior_gen_generic", "posterior_large", "posterior_gen_large"):
            out = {"mean": new(B, R), "var": new(B), "ykinvy": new(B, R)}
            args = head + model + (P(out["mean"]), P(out["var"]), P(out["ykinvy"]), P(info))
            if entry.endswith("large"):
                size = 2 * lib.mgp_large_workspace_bytes(es, k, R, 1)  # two slabs: every slab serves several neighbourhoods
                ws = torch.empty(size, dtype=torch.uint8, device=dev)
                args += (P(ws), size)
            rc = _lib.fn(entry, td)(*args, _lib.stream_ptr())
        else:
            gm, gv, gy = to(rng.normal(size=(B, R))), to(rng.normal(size=B)), to(rng.normal(size=B))
            out = {"grad_noise": new(B, k)}
            gls = None if opt.get("no_grad_ls") else new(B, ls.numel())
            if entry.endswith("large"):
                if gls is not None:
                    out["grad_ls"] = gls
                size = 2 * lib.mgp_backward_large_workspace_bytes(es, k, 1)
                ws = torch.empty(size, dtype=torch.uint8, device=dev)
                tail = (P(gls), P(out["grad_noise"]), P(info), P(ws), size, _lib.stream_ptr())
            else:
                tail = (P(gls), P(out["grad_noise"]), P(info), _lib.stream_ptr())
            sums = (new(N, d), new(N, d), new(N, R)) if opt.get("sweep") else (None, None, None)
            acc = tuple(P(t) for t in sums)
            if entry in ("loocv_backward", "posterior_backward"):
                # the LDS backward_kernel is what serves the shape: beyond the wave-sized backward (k + 2 > 64 rows) and
                # refused by the backward on the forward kernel
                assert k + 2 > 64 and lib.mgp_jit_prepare_backward(es, k, d, kid) == _lib.EUNSUPPORTED
            if entry == "hyper_backward_large":
                cot = (P(gm), P(gv), P(gy)) if opt["form"] == "loocv" else (P(gm), P(gv), None)
                rc = _lib.fn(entry, td)(P(Xn), d, P(bi), P(ni), B, k, P(Y), R, *model, *cot, *tail)
            elif entry == "loocv_backward":
                rc = _lib.fn(entry, td)(P(Xn), d, P(bi), P(ni), B, k, P(Y), *model, P(gm), P(gv), P(gy), *tail)
            else:  # posterior_backward, posterior_backward_large
                rc = _lib.fn(entry, td)(*head, *model, P(gm), P(gv), *acc, *tail)
    _lib.check(rc, f"{name}: mgp_{entry}")
    torch.cuda.synchronize()
    assert int(info.item()) == 0, f"{name}: {int(info.item())} systems were not positive definite"
    res = {n: t.cpu().numpy().tobytes() for n, t in out.items()}
    for n, raw in res.items():
        assert np.isfinite(np.frombuffer(raw, dtype=dtype)).all() and any(raw), f"{name}: {n} is empty or not finite"
    return res


def _encode(res):
    return {n: base64.b64encode(raw).decode() for n, raw in res.items()}


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", list(CASES))
def test_workgroup_kernel_bits_are_the_recorded_ones(name, dtype, golden):
    seen = run_case(name, dtype)
    want = {n: base64.b64decode(s) for n, s in golden[f"{name}/{dtype}"].items()}
    assert sorted(seen) == sorted(want)
    for n in sorted(seen):
        if seen[n] != want[n]:
            a, b = np.frombuffer(seen[n], dtype=dtype), np.frombuffer(want[n], dtype=dtype)
            bad = np.flatnonzero(a.view(f"u{a.itemsize}") != b.view(f"u{b.itemsize}"))
            pytest.fail(f"{name}/{dtype}: {n} differs in {bad.size} of {a.size} values, first at {bad[0]}: "
                        f"{a[bad[0]]!r} against the recorded {b[bad[0]]!r}")


if __name__ == "__main__":
    import argparse

    ap = argparse.ArgumentParser(description="record the bytes every case returns")
    ap.add_argument("--record", required=True, help="JSON file of the base64-encoded outputs")
    a = ap.parse_args()
    os.environ["MGP_BACKWARD_DLT"] = "0"  # (read once per process by the library: before the first call)
    record = {}
    for case in CASES:
        for dt in DTYPES:
            record[f"{case}/{dt}"] = _encode(run_case(case, dt))
            print(case, dt, {n: len(s) for n, s in record[f"{case}/{dt}"].items()}, flush=True)
    with open(a.record, "w") as f:
        json.dump(record, f, indent=0, sort_keys=True)
        f.write("\n")
