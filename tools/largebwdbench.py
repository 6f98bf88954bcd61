#!/usr/bin/env python
"""Timing of the hyper-parameter backward beyond LDS (csrc/mgp_backward_large.hip) next to the forward launch that
finite differences would repeat p + 1 times (csrc/mgp_large.hip) -> profiles/large_backward_bench.json.

Shapes: fp32 and fp64, Matern-3/2, d = 8, Isotropy and Anisotropy, nn_count in {mgp_max_nn_count_backward + 1, 256, 512,
1000}, one response, the LOOCV form (all three cotangents).  Per shape: the batch is sized from a trial forward launch so
that a launch takes tens of milliseconds; then, in one process and alternating, HIP events around one backward launch
(``mgp_hyper_backward_large_*`` through ``fused._hyper_partials``) and one forward launch
(``posterior_mean_var(path="large", want_ykinvy=True)``), median of 3 after a warm-up.  Recorded: both times and their
ratio -- an analytic gradient costs 1 + ratio forward launches where finite differences cost p + 1.

``--full``: the whole vector-Jacobian product beyond LDS (csrc/mgp_backward_large_full.hip) next to the hyper-parameter
backward at the same shape -> profiles/large_full_backward_bench.json.  The same shapes plus d = 40 at nn_count 256 and
1000 (where the per-point sweep and a second feature chunk show), the posterior form (grad_mean and grad_var), one
table on both sides.  Alternating in one process: one ``mgp_posterior_backward_large_*`` launch with every cotangent
(feature gradients into one shared buffer, responses, grad_ls, grad_noise) and one ``mgp_hyper_backward_large_*``
launch (grad_ls, grad_noise), HIP events, median of 3 after a warm-up.  Recorded: both times and their ratio.

Every shape runs in a child process of its own under a time limit: the parent never opens the GPU, and a shape that
fails or runs out of time ends the run there.

    python tools/largebwdbench.py [--full] [--out profiles/large_backward_bench.json] [--step-timeout 120]
"""

import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TARGET_MS = 40.0


def one(dtype: str, aniso: bool, k: int) -> dict:
    import torch

    from muygpys_amd import _lib, fused
    from muygpys_amd.fused import KernelSpec, posterior_mean_var

    t = getattr(torch, dtype)
    dev = torch.device("cuda:0")
    n, d = 20000, 8
    g = torch.Generator(device=dev).manual_seed(k * 100 + d + int(aniso))
    X = torch.rand((n, d), device=dev, dtype=t, generator=g)
    y = torch.sin(3.0 * X.sum(1)) + 0.1 * torch.randn(n, device=dev, dtype=t, generator=g)
    ls = [0.5 * (0.7 + 0.8 * i / (d - 1)) for i in range(d)] if aniso else 0.5
    spec = KernelSpec("matern15", "l2", ls, 1e-2)

    def indices(b):
        # distinct neighbours per row: k of a random permutation's window
        starts = torch.randint(0, n - k, (b, 1), device=dev, generator=g)
        return torch.randint(0, n, (b,), device=dev, generator=g), starts + torch.arange(k, device=dev)[None, :]

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    info = torch.zeros(1, dtype=torch.int32, device=dev)
    kernels = {}

    def launches(b):
        bi, ni = indices(b)
        inp = fused._normalize(spec, X, X, bi, ni, y, responses="single")
        cot = [torch.randn(b, device=dev, dtype=t, generator=g) for _ in range(3)]

        def forward():
            posterior_mean_var(spec, X, X, bi, ni, y, want_ykinvy=True, info=info, path="large", packed=False)
            kernels["forward"] = _lib.last_kernel()

        def backward():
            fused._hyper_partials(spec, inp, info, *cot)
            kernels["backward"] = _lib.last_kernel()

        return forward, backward

    trial_b = 256
    forward, _ = launches(trial_b)
    forward()
    trial = timed(forward)
    b = int(min(65536, max(64, trial_b * TARGET_MS / max(trial, 1e-3))))
    forward, backward = launches(b)
    times = {"forward": [], "backward": []}
    for i in range(4):  # (the first round is the warm-up)
        for name, fn in (("backward", backward), ("forward", forward)):
            ms = timed(fn)
            if i:
                times[name].append(ms)
    assert int(info.item()) == 0
    assert kernels["backward"].startswith("mgp::hyper_backward_large_kernel<"), kernels
    assert kernels["forward"].startswith("mgp::fused_large_kernel<"), kernels
    fwd, bwd = (sorted(times[name])[1] for name in ("forward", "backward"))
    return {"dtype": dtype, "d": d, "k": k, "anisotropic": aniso, "batch": b, "forward_ms": round(fwd, 3),
            "backward_ms": round(bwd, 3), "backward_over_forward": round(bwd / fwd, 3), **{f"{name}_kernel": v for name, v in kernels.items()}}


def one_full(dtype: str, aniso: bool, k: int, d: int) -> dict:
    """One shape of ``--full``: the whole backward against the hyper-parameter backward, both through the C entries."""
    import torch

    from muygpys_amd import _lib
    from muygpys_amd.fused import KernelSpec

    t = getattr(torch, dtype)
    dev = torch.device("cuda:0")
    n = 20000
    g = torch.Generator(device=dev).manual_seed(k * 100 + d + int(aniso))
    X = torch.rand((n, d), device=dev, dtype=t, generator=g)
    Y = (torch.sin(3.0 * X.sum(1)) + 0.1 * torch.randn(n, device=dev, dtype=t, generator=g)).reshape(n, 1).contiguous()
    ls = torch.tensor([0.5 * (0.7 + 0.8 * i / (d - 1)) for i in range(d)] if aniso else [0.5], device=dev, dtype=t)
    spec = KernelSpec("matern15", "l2", 1.0, 0.0)
    lib, P = _lib.load(), _lib.ptr
    info = torch.zeros(1, dtype=torch.int32, device=dev)
    g_x, g_t = torch.zeros_like(X), torch.zeros_like(Y)  # (accumulated into by every repetition: the values are not looked at)
    kernels = {}

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def launches(b):
        starts = torch.randint(0, n - k, (b, 1), device=dev, generator=g)
        bi, ni = torch.randint(0, n, (b,), device=dev, generator=g), (starts + torch.arange(k, device=dev)[None, :]).contiguous()
        gm, gv = torch.randn((b, 1), device=dev, dtype=t, generator=g), torch.randn(b, device=dev, dtype=t, generator=g)
        g_l, g_n = torch.empty((b, ls.numel()), device=dev, dtype=t), torch.empty((b, k), device=dev, dtype=t)
        ws = torch.empty(lib.mgp_backward_large_workspace_bytes(X.element_size(), k, b), dtype=torch.uint8, device=dev)
        shape = (d, P(bi), P(ni), b, k, P(Y), 1, 0, 1e-2, None, spec.kernel_id(), spec.metric_id(), P(ls), ls.numel(), P(gm), P(gv))
        tail = (P(g_l), P(g_n), P(info), P(ws), ws.numel(), _lib.stream_ptr())

        def full():
            rc = _lib.fn("posterior_backward_large", t)(P(X), P(X), *shape, P(g_x), P(g_x), P(g_t), *tail)
            assert rc == 0, rc
            kernels["full"] = _lib.last_kernel()

        def hyper():
            rc = _lib.fn("hyper_backward_large", t)(P(X), *shape, None, *tail)
            assert rc == 0, rc
            kernels["hyper"] = _lib.last_kernel()

        return full, hyper

    trial_b = 256
    _, hyper = launches(trial_b)
    hyper()
    trial = timed(hyper)
    b = int(min(65536, max(64, trial_b * TARGET_MS / max(trial, 1e-3))))
    full, hyper = launches(b)
    times = {"full": [], "hyper": []}
    for i in range(4):  # (the first round is the warm-up)
        for name, fn in (("full", full), ("hyper", hyper)):
            ms = timed(fn)
            if i:
                times[name].append(ms)
    assert int(info.item()) == 0
    assert kernels["full"].startswith("mgp::posterior_backward_large_kernel<"), kernels
    assert kernels["hyper"].startswith("mgp::hyper_backward_large_kernel<"), kernels
    f_ms, h_ms = (sorted(times[name])[1] for name in ("full", "hyper"))
    return {"dtype": dtype, "d": d, "k": k, "anisotropic": aniso, "batch": b, "hyper_ms": round(h_ms, 3), "full_ms": round(f_ms, 3),
            "full_over_hyper": round(f_ms / h_ms, 3), **{f"{name}_kernel": v for name, v in kernels.items()}}


def main_full(a, lib):
    records = []
    for dtype, es in (("float32", 4), ("float64", 8)):
        first = lib.mgp_max_nn_count_backward(es) + 1
        shapes = [(aniso, k, 8) for aniso in (False, True) for k in (first, 256, 512, 1000)]
        shapes += [(aniso, k, 40) for aniso in (False, True) for k in (256, 1000)]
        for aniso, k, d in shapes:
            cmd = [sys.executable, os.path.abspath(__file__), "--one-full", dtype, "1" if aniso else "0", str(k), str(d)]
            what = f"{dtype} {'Anisotropy' if aniso else 'Isotropy'} k={k} d={d}"
            try:
                r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=a.step_timeout)
            except subprocess.TimeoutExpired:
                print(f"largebwdbench: {what} ran out of its {a.step_timeout:.0f} s; stopping", file=sys.stderr)
                return 1
            if r.returncode != 0:
                print(f"largebwdbench: {what} failed ({r.returncode}); stopping\n{r.stderr[-2000:]}", file=sys.stderr)
                return 1
            rec = json.loads(r.stdout.strip().splitlines()[-1])
            print(json.dumps(rec), flush=True)
            records.append(rec)
    out = a.out or os.path.join(ROOT, "profiles", "large_full_backward_bench.json")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump({"full": "mgp_posterior_backward_large_*, every cotangent, one table on both sides",
                   "hyper": "mgp_hyper_backward_large_*, posterior form, grad_ls + grad_noise", "shapes": records}, f, indent=1)
        f.write("\n")
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="default: profiles/large_backward_bench.json (--full: profiles/large_full_backward_bench.json)")
    ap.add_argument("--step-timeout", type=float, default=120.0)
    ap.add_argument("--full", action="store_true", help="the whole backward against the hyper-parameter backward")
    ap.add_argument("--one", nargs=3, metavar=("DTYPE", "ANISO", "K"), help="(child) time one shape and print its record")
    ap.add_argument("--one-full", nargs=4, metavar=("DTYPE", "ANISO", "K", "D"), help="(child of --full) likewise")
    a = ap.parse_args()
    if a.one:
        print(json.dumps(one(a.one[0], a.one[1] == "1", int(a.one[2]))), flush=True)
        return 0
    if a.one_full:
        print(json.dumps(one_full(a.one_full[0], a.one_full[1] == "1", int(a.one_full[2]), int(a.one_full[3]))), flush=True)
        return 0
    import ctypes

    from muygpys_amd import _abi

    lib = _abi.bind(ctypes.CDLL(os.path.join(ROOT, "muygpys_amd", "lib", "libmuygpys_hip.so")))  # (no GPU is opened here)
    if a.full:
        return main_full(a, lib)
    a.out = a.out or os.path.join(ROOT, "profiles", "large_backward_bench.json")
    records = []
    for dtype, es in (("float32", 4), ("float64", 8)):
        first = lib.mgp_max_nn_count_backward(es) + 1
        for aniso in (False, True):
            for k in (first, 256, 512, 1000):
                cmd = [sys.executable, os.path.abspath(__file__), "--one", dtype, "1" if aniso else "0", str(k)]
                what = f"{dtype} {'Anisotropy' if aniso else 'Isotropy'} k={k}"
                try:
                    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=a.step_timeout)
                except subprocess.TimeoutExpired:
                    print(f"largebwdbench: {what} ran out of its {a.step_timeout:.0f} s; stopping", file=sys.stderr)
                    return 1
                if r.returncode != 0:
                    print(f"largebwdbench: {what} failed ({r.returncode}); stopping\n{r.stderr[-2000:]}", file=sys.stderr)
                    return 1
                rec = json.loads(r.stdout.strip().splitlines()[-1])
                print(json.dumps(rec), flush=True)
                records.append(rec)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"forward": "posterior_mean_var(path='large', want_ykinvy=True)", "backward": "mgp_hyper_backward_large_*, LOOCV form",
                   "shapes": records}, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
