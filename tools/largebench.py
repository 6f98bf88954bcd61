#!/usr/bin/env python
"""Timing of the blocked factorisation beyond LDS (csrc/mgp_large.hip) -> profiles/large_bench.json.

Shapes: fp32 and fp64, Matern-3/2, d = 8 and d = 40, nn_count in {the largest mgp_max_nn_count allows, 256, 512, 1000},
one response.  Per shape: the batch is sized from a trial launch so that one launch takes tens of milliseconds, then
HIP events around single launches, median of 3 after a warm-up.  Recorded: neighbourhoods/s, achieved FLOP/s on
k^3 / 3 + k^2 (1 + R) against the fp32 / fp64 vector peak, and -- at the one nn_count both kernels serve -- the time of
path="generic" next to path="large".

Every shape runs in a child process of its own under a time limit: the parent never opens the GPU, and a shape that
fails or runs out of time ends the run there.

    python tools/largebench.py [--out profiles/large_bench.json] [--step-timeout 120]
"""

import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK = {"float32": 157.3e12, "float64": 78.6e12}  # vector peaks of the MI355X (the exact matrix forms issue at the same rate)
TARGET_MS = 40.0


def flops(k, R=1):
    return k**3 / 3.0 + k * k * (1.0 + R)


def one(dtype: str, d: int, k: int, both: bool) -> dict:
    import torch

    from muygpys_amd import _lib
    from muygpys_amd.fused import KernelSpec, posterior_mean_var

    t = getattr(torch, dtype)
    dev = torch.device("cuda:0")
    n = 20000
    g = torch.Generator(device=dev).manual_seed(k * 100 + d)
    X = torch.rand((n, d), device=dev, dtype=t, generator=g)
    y = torch.sin(3.0 * X.sum(1)) + 0.1 * torch.randn(n, device=dev, dtype=t, generator=g)
    spec = KernelSpec("matern15", "l2", 0.5, 1e-2)

    def indices(b):
        # distinct neighbours per row: k of a random permutation's window
        starts = torch.randint(0, n - k, (b, 1), device=dev, generator=g)
        return torch.randint(0, n, (b,), device=dev, generator=g), starts + torch.arange(k, device=dev)[None, :]

    def time_ms(path, b, reps):
        bi, ni = indices(b)
        info = torch.zeros(1, dtype=torch.int32, device=dev)
        times = []
        for i in range(reps + 1):  # (the first launch is the warm-up)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            posterior_mean_var(spec, X, X, bi, ni, y, want_ykinvy=True, info=info, path=path, packed=False)
            e1.record()
            e1.synchronize()
            if i:
                times.append(e0.elapsed_time(e1))
        assert int(info.item()) == 0
        return sorted(times)[len(times) // 2], _lib.last_kernel()

    out = {"dtype": dtype, "d": d, "k": k, "R": 1}
    for path in ("large", "generic") if both else ("large",):
        trial_b = 256
        trial, _ = time_ms(path, trial_b, 1)
        b = int(min(65536, max(64, trial_b * TARGET_MS / max(trial, 1e-3))))
        ms, kernel = time_ms(path, b, 3)
        rate = b / (ms * 1e-3)
        out[path] = {"kernel": kernel, "batch": b, "ms": round(ms, 3), "nbhd_per_s": round(rate, 1),
                     "flop_per_s": round(rate * flops(k), 1), "fraction_of_vector_peak": round(rate * flops(k) / PEAK[dtype], 4)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "large_bench.json"))
    ap.add_argument("--step-timeout", type=float, default=120.0)
    ap.add_argument("--one", nargs=4, metavar=("DTYPE", "D", "K", "BOTH"), help="(child) time one shape and print its record")
    a = ap.parse_args()
    if a.one:
        print(json.dumps(one(a.one[0], int(a.one[1]), int(a.one[2]), a.one[3] == "1")), flush=True)
        return 0
    import ctypes

    from muygpys_amd import _abi

    lib = _abi.bind(ctypes.CDLL(os.path.join(ROOT, "muygpys_amd", "lib", "libmuygpys_hip.so")))  # (no GPU is opened here)
    records = []
    for dtype, es in (("float32", 4), ("float64", 8)):
        kmax = lib.mgp_max_nn_count(es, 1)
        for d in (8, 40):
            for k in (kmax, 256, 512, 1000):
                cmd = [sys.executable, os.path.abspath(__file__), "--one", dtype, str(d), str(k), "1" if k == kmax else "0"]
                try:
                    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=a.step_timeout)
                except subprocess.TimeoutExpired:
                    print(f"largebench: {dtype} d={d} k={k} ran out of its {a.step_timeout:.0f} s; stopping", file=sys.stderr)
                    return 1
                if r.returncode != 0:
                    print(f"largebench: {dtype} d={d} k={k} failed ({r.returncode}); stopping\n{r.stderr[-2000:]}", file=sys.stderr)
                    return 1
                rec = json.loads(r.stdout.strip().splitlines()[-1])
                print(json.dumps(rec), flush=True)
                records.append(rec)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"peak_flop_per_s": PEAK, "flops_per_neighbourhood": "k^3 / 3 + k^2 (1 + R)", "shapes": records}, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
