#!/usr/bin/env python3
"""Throughput of the fast-posterior-mean workflow (GPU box only).

    python tools/fastbench.py                # the prediction kernel at the headline shape (k = 30, d = 40)
    python tools/fastbench.py --beyond64     # nn_count > 64: coefficient precompute and prediction kernel, fused against
                                             # the materialising routes -> profiles/fast_beyond64_bench.json
    python tools/fastbench.py --gen          # the general-smoothness Matern (nu = 1.3): fused.gen_fast("fused") against the
                                             # materialised route and the closed-form launches -> profiles/fast_gen_bench.json
    python tools/fastbench.py --gen --only coefficients:float32    # one part of it (a part per process under its own timeout)

Timing: HIP events around the call, warm-up calls first, median of the repeats, the spread (min, max) reported.
--gen: the routes under comparison alternate in one process, each call between two device synchronisations on the host
clock, a warm-up call per route and shape, median of the repeats, min / max kept."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from bench import random_neighbors, synth
from muygpys_amd.fused import KernelSpec, fast_coefficients, fast_posterior_mean

dev = torch.device("cuda")
PEAK_GBS = 8000.0  # HBM of an MI355X, GB/s


def timed(fn, warmup=1, repeats=3):
    """{median, min, max} ms of ``fn()`` by HIP events, after ``warmup`` calls."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return dict(median_ms=float(np.median(ts)), min_ms=float(min(ts)), max_ms=float(max(ts)), repeats=repeats, warmup=warmup)


def headline():
    n, b, k, d = 1_000_000, 1_000_000, 30, 40
    X, y = synth(n, d, 20241008)
    Xd = torch.from_numpy(X).to(dev)
    _, ni = random_neighbors(n, b, k, 1)
    ni = torch.from_numpy(ni).to(dev)
    coeffs = torch.randn((n, k), device=dev)
    closest = torch.randint(0, n, (b,), device=dev)
    spec = KernelSpec("matern15", "l2", 5.0, 1e-3)
    out = torch.empty((b, 1), device=dev)
    t = timed(lambda: fast_posterior_mean(spec, Xd, Xd, None, ni, coeffs, closest, out=out), warmup=2, repeats=6)["median_ms"]
    B = (k + 1) * d * 4 + k * 4 + 8 * (k + 2) + 4
    print(f"fast posterior mean: {t:.3f} ms -> {b / t / 1e3:.1f} M test points/s, {B} B/point algorithmic -> "
          f"{B * b / t / 1e6:.0f} GB/s = {B * b / t / 1e6 / PEAK_GBS:.1%} of 8 TB/s")


def precompute_rows():
    """Coefficient precompute, one fused launch against the chunked materialising route (fused=False)."""
    rows = []
    for k, d, n in ((100, 40, 200_000), (300, 8, 20_000)):
        g = torch.Generator().manual_seed(k)
        X64 = torch.rand(n, d, generator=g, dtype=torch.float64)
        Y64 = torch.sin(3.0 * X64.sum(1))[:, None] + 0.1 * torch.randn(n, 3, generator=g, dtype=torch.float64)
        nn = torch.randint(0, n, (n, k), generator=g).to(dev)
        spec = KernelSpec("matern15", "l2", 0.5 * (d / 8.0) ** 0.5, 1e-2)
        for dtype in (torch.float32, torch.float64):
            Xd = X64.to(dev, dtype)
            for R in (1, 3):
                Yd = (Y64[:, 0] if R == 1 else Y64).to(dev, dtype).contiguous()
                row = dict(k=k, d=d, n=n, dtype=str(dtype).split(".")[1], R=R)
                for name, fused in (("fused", True), ("materialising", False)):
                    torch.cuda.synchronize()
                    torch.cuda.reset_peak_memory_stats()
                    base = torch.cuda.memory_allocated()
                    row[name] = timed(lambda: fast_coefficients(spec, Xd, Yd, nn, fused=fused))
                    row[name]["peak_bytes"] = int(torch.cuda.max_memory_allocated() - base)
                    torch.cuda.empty_cache()
                row["speedup"] = row["materialising"]["median_ms"] / row["fused"]["median_ms"]
                print(json.dumps(row), flush=True)
                rows.append(row)
    return rows


def prediction_rows():
    """The prediction kernel against materialised Kcross + einsum, as GB/s of the algorithmic bytes
    (k+1) d s + k R s + 8 (k+2) + R s per test point."""
    from muygpys_amd._src.gp.kernels import hip as K
    from muygpys_amd._src.gp.tensors import hip as T

    rows = []
    n, d, R, s = 200_000, 40, 1, 4
    g = torch.Generator().manual_seed(7)
    Xd = torch.rand(n, d, generator=g).to(dev)
    spec = KernelSpec("matern15", "l2", 1.1, 0.0)
    for k in (64, 100, 300, 1023):
        b = 200_000 if k <= 300 else 50_000
        ni = torch.randint(0, n, (b, k), generator=g).to(dev)
        bi = torch.arange(b, device=dev)
        coeffs = torch.randn((b, k), generator=g).to(dev)
        crow = torch.randperm(b, generator=g).to(dev)
        out = torch.empty((b, R), device=dev)
        fused_t = timed(lambda: fast_posterior_mean(spec, Xd, Xd, bi, ni, coeffs, crow, out=out), warmup=2, repeats=5)

        def materialised():
            Kc = K._apply(T._crosswise_distances(Xd, Xd, bi, ni, "l2"), "matern15", 1.0 / 1.1)
            return torch.einsum("ij,ij->i", Kc, coeffs[crow])

        mat_t = timed(materialised, warmup=2, repeats=5)
        bytes_pt = (k + 1) * d * s + k * R * s + 8 * (k + 2) + R * s
        row = dict(k=k, d=d, b=b, R=R, dtype="float32", bytes_per_point=bytes_pt, fused=fused_t, materialised=mat_t)
        for name in ("fused", "materialised"):
            gbs = bytes_pt * b / row[name]["median_ms"] / 1e6
            row[name]["algorithmic_GBs"] = gbs
            row[name]["fraction_of_8TBs"] = gbs / PEAK_GBS
        print(json.dumps(row), flush=True)
        rows.append(row)
    return rows


# ---- the general-smoothness Matern: fused.gen_fast("fused") against what it replaces ------------------------------------
GEN_NU = 1.3


def alternating(routes, warmup=1, repeats=3):
    """{route: {median_ms, min_ms, max_ms, peak_bytes}}: the routes take turns, one call each per round, every call
    between two device synchronisations on the host clock; a warm-up call each first; the peak allocation of one more
    call each afterwards."""
    for fn in routes.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    ts = {name: [] for name in routes}
    for _ in range(repeats):
        for name, fn in routes.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts[name].append((time.perf_counter() - t0) * 1e3)
    out = {}
    for name, fn in routes.items():
        torch.cuda.empty_cache()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        fn()
        torch.cuda.synchronize()
        out[name] = dict(median_ms=float(np.median(ts[name])), min_ms=float(min(ts[name])), max_ms=float(max(ts[name])),
                         repeats=repeats, warmup=warmup, peak_bytes=int(torch.cuda.max_memory_allocated() - base))
    torch.cuda.empty_cache()
    return out


def closed_form_workgroup_coefficients(spec, Xd, Yd, nn_fast):
    """``mgp_fast_coefficients_any_*`` called directly (the closed-form launch of the kernel family the general-nu
    entry uses; ``fused.fast_coefficients`` would take the wave entry at k <= 62)."""
    from muygpys_amd import _lib
    from muygpys_amd.fused import _normalize

    P = _lib.ptr
    inp = _normalize(spec, Xd, Xd, None, nn_fast, Yd)
    out = torch.empty((inp.b, inp.k, inp.R), device=dev, dtype=Xd.dtype)
    info = torch.zeros(1, device=dev, dtype=torch.int32)
    ws = _lib.workspace("mgp_fast_coefficients_workspace_bytes", Xd.dtype, inp.k, inp.R, inp.b, device=dev)
    rc = _lib.fn("fast_coefficients_any", Xd.dtype)(
        P(inp.fn), inp.d, P(inp.ni), inp.b, inp.k, P(inp.tg), inp.R, inp.mode, inp.eps, P(inp.nz), spec.kernel_id(), spec.metric_id(),
        P(inp.ls), inp.ls.numel(), P(out), P(info), P(ws), 0 if ws is None else ws.numel(), _lib.stream_ptr())
    _lib.check(rc, "mgp_fast_coefficients_any")
    return out


def gen_coefficient_rows(dtype):
    from muygpys_amd import fused
    from muygpys_amd._src.gp.tensors import hip as T

    rows = []
    for k, d, n in ((30, 40, 200_000), (100, 40, 200_000), (300, 8, 20_000)):
        g = torch.Generator().manual_seed(k)
        Xd = torch.rand(n, d, generator=g, dtype=torch.float64).to(dev, dtype)
        Yd = (torch.sin(3.0 * Xd.double().sum(1)) + 0.1 * torch.randn(n, generator=g, dtype=torch.float64).to(dev)).to(dtype)
        nn = torch.randint(0, n, (n, k), generator=g).to(dev)
        nn_fast = T._fast_nn_update(nn)
        ell = 0.5 * (d / 8.0) ** 0.5
        gen = KernelSpec("matern_gen", "l2", ell, 1e-2, smoothness=GEN_NU)
        closed = KernelSpec("matern15", "l2", ell, 1e-2)

        def fused_gen():
            with fused.gen_fast("fused"):
                return fast_coefficients(gen, Xd, Yd, nn)

        routes = {"fused": fused_gen,
                  "materialised": lambda: fast_coefficients(gen, Xd, Yd, nn, fused=False),
                  "closed_form_same_family": lambda: closed_form_workgroup_coefficients(closed, Xd, Yd, nn_fast)}
        if k <= 62:  # (what serving k <= 62 from the workgroup kernel costs against a wave kernel)
            routes["closed_form_wave_entry"] = lambda: fast_coefficients(closed, Xd, Yd, nn)
        row = dict(k=k, d=d, n=n, R=1, dtype=str(dtype).split(".")[1], nu=GEN_NU, **alternating(routes, repeats=5))
        row["fused_over_materialised"] = row["materialised"]["median_ms"] / row["fused"]["median_ms"]
        row["fused_over_closed_form"] = row["fused"]["median_ms"] / row["closed_form_same_family"]["median_ms"]
        print(json.dumps(row), flush=True)
        rows.append(row)
    return rows


def gen_prediction_rows(dtype):
    from muygpys_amd import fused
    from muygpys_amd._src.gp.kernels import hip as K
    from muygpys_amd._src.gp.tensors import hip as T

    rows = []
    n, d, R = 200_000, 40, 1
    s = 4 if dtype == torch.float32 else 8
    ell = 1.1
    g = torch.Generator().manual_seed(7)
    Xd = torch.rand(n, d, generator=g).to(dev, dtype)
    gen = KernelSpec("matern_gen", "l2", ell, 0.0, smoothness=GEN_NU)
    closed = KernelSpec("matern15", "l2", ell, 0.0)
    for k in (30, 64, 100, 300, 1023):
        b = 200_000 if k <= 300 else 50_000
        ni = torch.randint(0, n, (b, k), generator=g).to(dev)
        bi = torch.arange(b, device=dev)
        coeffs = torch.randn((b, k), generator=g).to(dev, dtype)
        crow = torch.randperm(b, generator=g).to(dev)
        out = torch.empty((b, R), device=dev, dtype=dtype)

        def fused_gen():
            with fused.gen_fast("fused"):
                return fast_posterior_mean(gen, Xd, Xd, bi, ni, coeffs, crow, out=out)

        def materialised():  # Kcross (b, k), the Bessel form element-wise, the gathered coefficient copy, the einsum
            Kc = K._matern_gen_fn(T._crosswise_distances(Xd, Xd, bi, ni, "l2") * (1.0 / ell), GEN_NU)
            return torch.einsum("ij,ij->i", Kc, coeffs[crow])

        routes = {"fused": fused_gen, "materialised": materialised,
                  "closed_form": lambda: fast_posterior_mean(closed, Xd, Xd, bi, ni, coeffs, crow, out=out)}
        bytes_pt = (k + 1) * d * s + k * R * s + 8 * (k + 2) + R * s
        row = dict(k=k, d=d, b=b, R=R, dtype=str(dtype).split(".")[1], nu=GEN_NU, bytes_per_point=bytes_pt, **alternating(routes, repeats=5))
        for name in routes:
            gbs = bytes_pt * b / row[name]["median_ms"] / 1e6
            row[name]["algorithmic_GBs"] = gbs
            row[name]["fraction_of_8TBs"] = gbs / PEAK_GBS
        row["fused_over_materialised"] = row["materialised"]["median_ms"] / row["fused"]["median_ms"]
        row["fused_over_closed_form"] = row["fused"]["median_ms"] / row["closed_form"]["median_ms"]
        print(json.dumps(row), flush=True)
        rows.append(row)
    return rows


GEN_PARTS = {f"{what}:{dt}": (fn, getattr(torch, dt)) for what, fn in (("coefficients", gen_coefficient_rows), ("prediction", gen_prediction_rows))
             for dt in ("float32", "float64")}


def gen_bench(out_path, only=None):
    """Every part (or the one named), merged into ``out_path``: a part per process lets each run under its own timeout."""
    from muygpys_amd import _lib

    result = {}
    if os.path.exists(out_path):
        with open(out_path) as f:
            result = json.load(f)
    result.update(device=torch.cuda.get_device_name(0), nu=GEN_NU,
                  method="routes alternate in one process; each call between two device synchronisations on the host clock; "
                         "one warm-up call per route and shape; median of the repeats (min / max kept); peak_bytes: "
                         "torch's peak allocation over one more call",
                  max_nn_count_gen={"float32": _lib.load().mgp_max_nn_count_gen(4, 1), "float64": _lib.load().mgp_max_nn_count_gen(8, 1)})
    for name in ([only] if only else sorted(GEN_PARTS)):
        fn, dtype = GEN_PARTS[name]
        result[name] = fn(dtype)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", out_path)


def beyond64(out_path):
    from muygpys_amd import _lib

    result = dict(
        device=torch.cuda.get_device_name(0), method="HIP events, warm-up calls, median of the repeats (min / max kept)",
        max_nn_count={"float32": _lib.load().mgp_max_nn_count(4, 1), "float64": _lib.load().mgp_max_nn_count(8, 1)},
        prediction=prediction_rows(), precompute=precompute_rows(),
    )
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", out_path)


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--beyond64", action="store_true")
    ap.add_argument("--gen", action="store_true")
    ap.add_argument("--only", choices=sorted(GEN_PARTS), default=None, help="--gen: one part (merged into the output file)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    profiles = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles")
    a.out = a.out or os.path.join(profiles, "fast_gen_bench.json" if a.gen else "fast_beyond64_bench.json")
    if a.gen:
        gen_bench(a.out, a.only)
    elif a.beyond64:
        beyond64(a.out)
    else:
        headline()
