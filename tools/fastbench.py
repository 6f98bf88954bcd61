#!/usr/bin/env python3
"""Throughput of the fast-posterior-mean workflow (GPU box only).

    python tools/fastbench.py                # the prediction kernel at the headline shape (k = 30, d = 40)
    python tools/fastbench.py --beyond64     # nn_count > 64: coefficient precompute and prediction kernel, fused against
                                             # the materialising routes -> profiles/fast_beyond64_bench.json

Timing: HIP events around the call, warm-up calls first, median of the repeats, the spread (min, max) reported."""
import argparse
import json
import os
import sys

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
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "fast_beyond64_bench.json"))
    a = ap.parse_args()
    if a.beyond64:
        beyond64(a.out)
    else:
        headline()
