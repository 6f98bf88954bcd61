#!/usr/bin/env python
"""Timing of the hyper-parameter backward of the general-smoothness Matern (csrc/mgp_backward_gen_large.hip) next to
the forward launch that finite differences would repeat p + 1 times -> profiles/gen_backward_bench.json.

Shapes: (nn_count, features, neighbourhoods) = (30, 40, 200 000), (100, 40, 200 000), (300, 8, 20 000), each in fp32 and
fp64, nu = 1.3, Isotropy, l2, one response, the LOOCV form (all three cotangents), a table of 20 000 points.  Per shape,
in one process and alternating after a warm-up round, HIP events around

    forward          the general-nu forward launch (``posterior_mean_var(..., want_ykinvy=True)``: a wave kernel up to
                     64 slots, the LDS workgroup kernel or the slab kernel beyond)
    backward         ``mgp_hyper_backward_gen_large_*`` with grad_ls and grad_noise
    backward_nu      ... and grad_nu (three exponentials per quadrature node and pair instead of one)
    closed_form      ``mgp_hyper_backward_large_*`` with MGP_KERNEL_MATERN_15 on the same inputs: the same slab kernel
                     around a closed-form kernel function

median of 5 rounds, with the smallest and the largest; then the ratios backward / forward.  An analytic gradient costs
1 + ratio forward launches where finite differences cost p + 1: it pays from p > ratio free parameters.

Every shape runs in a child process of its own under a time limit: the parent never opens the GPU, and a shape that
fails or runs out of time ends the run there.

    python tools/genbwdbench.py [--out profiles/gen_backward_bench.json] [--step-timeout 150]

``--lds``: the LDS workgroup backward (csrc/mgp_backward_gen.hip, ``mgp_posterior_backward_gen_*``) against the slab
backward at the same shape, in the same process, alternating launches -> profiles/gen_backward_lds_bench.json.
Shapes: nn_count = 30, 63 and 100 at d = 40, 200 000 neighbourhoods, otherwise as above.  Per shape and width

    forward, slab, slab_nu      as forward / backward / backward_nu above
    lds, lds_nu                 ``mgp_posterior_backward_gen_*`` with grad_ls and grad_noise, without / with grad_nu
    lds_full                    ... with every cotangent: both feature tables, the responses, grad_ls, grad_noise, grad_nu

median, smallest and largest of 3 alternating rounds after a warm-up; ``lds_wins`` / ``lds_nu_wins``: the LDS kernel's
largest time is below the slab's smallest (faster by more than the spread of the repeats).  A shape beyond
``mgp_max_nn_count_backward_gen`` is recorded as refused.
"""

import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(30, 40, 200000), (100, 40, 200000), (300, 8, 20000)]
NU, ROUNDS = 1.3, 5


def one(dtype: str, k: int, d: int, b: int) -> dict:
    import statistics

    import torch

    from muygpys_amd import _lib
    from muygpys_amd.fused import FusedUnsupported, KernelSpec, posterior_mean_var

    t = getattr(torch, dtype)
    dev = torch.device("cuda:0")
    n = 20000
    g = torch.Generator(device=dev).manual_seed(k * 100 + d)
    X = torch.rand((n, d), device=dev, dtype=t, generator=g)
    y = (torch.sin(3.0 * X.sum(1)) + 0.1 * torch.randn(n, device=dev, dtype=t, generator=g)).reshape(n, 1).contiguous()
    ell = 0.5 * max(1.0, (d / 8.0) ** 0.5)
    spec = KernelSpec("matern_gen", "l2", ell, 1e-2, smoothness=NU)
    # distinct neighbours per row: a window of k rows of the table
    starts = torch.randint(0, n - k, (b, 1), device=dev, generator=g)
    bi = torch.randint(0, n, (b,), device=dev, generator=g)
    ni = (starts + torch.arange(k, device=dev)[None, :]).contiguous()
    cot = [torch.randn(b, device=dev, dtype=t, generator=g) for _ in range(3)]
    ls = torch.tensor([ell], device=dev, dtype=t)
    P, lib = _lib.ptr, _lib.load()
    ws = torch.empty(lib.mgp_backward_large_workspace_bytes(X.element_size(), k, b), dtype=torch.uint8, device=dev)
    g_l = torch.zeros((b, 1), device=dev, dtype=t)
    g_n = torch.zeros((b, k), device=dev, dtype=t)
    g_nu = torch.zeros((b,), device=dev, dtype=t)
    info = torch.zeros(1, dtype=torch.int32, device=dev)
    head = (P(X), d, P(bi), P(ni), b, k, P(y), 1, 0, 1e-2, None)
    tail = (P(ls), 1, *[P(c) for c in cot], P(g_l), P(g_n))
    kernels = {}

    path = {"name": "auto"}

    def forward():
        posterior_mean_var(spec, X, X, bi, ni, y, want_ykinvy=True, packed=False, path=path["name"])

    try:  # (up to 64 slots the wave kernels serve fp64 on their static shapes only: the slab kernel where they refuse)
        forward()
    except FusedUnsupported:
        path["name"] = "large"

    def backward(nu_out):
        def run():
            rc = _lib.fn("hyper_backward_gen_large", t)(*head, NU, 0, *tail, P(g_nu) if nu_out else None, P(info), P(ws),
                                                        ws.numel(), _lib.stream_ptr())
            _lib.check(rc, "mgp_hyper_backward_gen_large")
        return run

    def closed_form():
        rc = _lib.fn("hyper_backward_large", t)(*head, _lib.KERNEL_IDS["matern15"], 0, *tail, P(info), P(ws), ws.numel(),
                                                _lib.stream_ptr())
        _lib.check(rc, "mgp_hyper_backward_large")

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    what = {"forward": forward, "backward": backward(False), "backward_nu": backward(True), "closed_form": closed_form}
    for name, fn in what.items():  # warm-up: code objects loaded, every buffer touched
        timed(fn)
        kernels[name] = _lib.last_kernel()
    times = {name: [] for name in what}
    for _ in range(ROUNDS):
        for name, fn in what.items():
            times[name].append(timed(fn))
    assert int(info.item()) == 0, "a neighbourhood did not factorise"
    out = {"dtype": dtype, "nn_count": k, "features": d, "neighbourhoods": b, "smoothness": NU, "forward_path": path["name"],
           "kernels": kernels}
    for name, v in times.items():
        out[name + "_ms"] = {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}
    fwd = out["forward_ms"]["median"]
    for name in ("backward", "backward_nu", "closed_form"):
        out[name + "_over_forward"] = round(out[name + "_ms"]["median"] / fwd, 2)
    return out


LDS_SHAPES = [(30, 40, 200000), (63, 40, 200000), (100, 40, 200000)]
LDS_ROUNDS = 3


def one_lds(dtype: str, k: int, d: int, b: int) -> dict:
    import statistics

    import torch

    from muygpys_amd import _lib
    from muygpys_amd.fused import FusedUnsupported, KernelSpec, posterior_mean_var

    t = getattr(torch, dtype)
    dev = torch.device("cuda:0")
    n = 20000
    g = torch.Generator(device=dev).manual_seed(k * 100 + d)
    X = torch.rand((n, d), device=dev, dtype=t, generator=g)
    y = (torch.sin(3.0 * X.sum(1)) + 0.1 * torch.randn(n, device=dev, dtype=t, generator=g)).reshape(n, 1).contiguous()
    ell = 0.5 * max(1.0, (d / 8.0) ** 0.5)
    spec = KernelSpec("matern_gen", "l2", ell, 1e-2, smoothness=NU)
    starts = torch.randint(0, n - k, (b, 1), device=dev, generator=g)
    bi = torch.randint(0, n, (b,), device=dev, generator=g)
    ni = (starts + torch.arange(k, device=dev)[None, :]).contiguous()
    cot = [torch.randn(b, device=dev, dtype=t, generator=g) for _ in range(3)]
    ls = torch.tensor([ell], device=dev, dtype=t)
    P, lib = _lib.ptr, _lib.load()
    ws = torch.empty(lib.mgp_backward_large_workspace_bytes(X.element_size(), k, b), dtype=torch.uint8, device=dev)
    g_l = torch.zeros((b, 1), device=dev, dtype=t)
    g_n = torch.zeros((b, k), device=dev, dtype=t)
    g_nu = torch.zeros((b,), device=dev, dtype=t)
    g_x, g_t = torch.zeros_like(X), torch.zeros_like(y)
    info = torch.zeros(1, dtype=torch.int32, device=dev)
    shape = (d, P(bi), P(ni), b, k, P(y), 1, 0, 1e-2, None, NU, 0, P(ls), 1, *[P(c) for c in cot])
    limit = int(lib.mgp_max_nn_count_backward_gen(X.element_size()))
    path = {"name": "auto"}

    def forward():
        posterior_mean_var(spec, X, X, bi, ni, y, want_ykinvy=True, packed=False, path=path["name"])

    try:
        forward()
    except FusedUnsupported:
        path["name"] = "large"

    def slab(nu_out):
        def run():
            rc = _lib.fn("hyper_backward_gen_large", t)(P(X), *shape, P(g_l), P(g_n), P(g_nu) if nu_out else None, P(info),
                                                        P(ws), ws.numel(), _lib.stream_ptr())
            _lib.check(rc, "mgp_hyper_backward_gen_large")
        return run

    def lds(nu_out, full=False):
        def run():
            feat = (P(g_x), P(g_x), P(g_t)) if full else (None, None, None)
            rc = _lib.fn("posterior_backward_gen", t)(P(X), P(X), *shape, *feat, P(g_l), P(g_n), P(g_nu) if nu_out else None,
                                                      P(info), _lib.stream_ptr())
            _lib.check(rc, "mgp_posterior_backward_gen")
        return run

    what = {"forward": forward, "slab": slab(False), "slab_nu": slab(True)}
    if k <= limit:
        what.update(lds=lds(False), lds_nu=lds(True), lds_full=lds(True, True))

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    kernels, geometry = {}, {}
    for name, fn in what.items():  # warm-up: code objects loaded, every buffer touched
        timed(fn)
        kernels[name] = _lib.last_kernel()
        if name.startswith("lds"):
            geometry[name] = dict(zip(("workgroups", "lds_bytes"), _lib.last_launch_geometry()))
    times = {name: [] for name in what}
    for _ in range(LDS_ROUNDS):
        for name, fn in what.items():
            times[name].append(timed(fn))
    assert int(info.item()) == 0, "a neighbourhood did not factorise"
    out = {"dtype": dtype, "nn_count": k, "features": d, "neighbourhoods": b, "smoothness": NU, "forward_path": path["name"],
           "lds_limit": limit, "kernels": kernels, "lds_geometry": geometry}
    for name, v in times.items():
        out[name + "_ms"] = {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}
    fwd = out["forward_ms"]["median"]
    for name in times:
        if name != "forward":
            out[name + "_over_forward"] = round(out[name + "_ms"]["median"] / fwd, 2)
    if k <= limit:
        for a_, b_ in (("lds", "slab"), ("lds_nu", "slab_nu")):
            out[a_ + "_wins"] = out[a_ + "_ms"]["max"] < out[b_ + "_ms"]["min"]
            out[b_ + "_over_" + a_] = round(out[b_ + "_ms"]["median"] / out[a_ + "_ms"]["median"], 2)
    else:
        out["lds"] = f"refused: nn_count beyond mgp_max_nn_count_backward_gen = {limit}"
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lds", action="store_true", help="the LDS backward against the slab backward (see the module docstring)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--step-timeout", type=int, default=150)
    ap.add_argument("--one", nargs=4, metavar=("DTYPE", "K", "D", "B"))
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "gen_backward_lds_bench.json" if a.lds else "gen_backward_bench.json")
    if a.one:
        fn = one_lds if a.lds else one
        print("RESULT " + json.dumps(fn(a.one[0], int(a.one[1]), int(a.one[2]), int(a.one[3]))), flush=True)
        return 0
    rows = []
    for k, d, b in (LDS_SHAPES if a.lds else SHAPES):
        for dtype in ("float32", "float64"):
            cmd = [sys.executable, os.path.abspath(__file__), *(["--lds"] if a.lds else []), "--one", dtype, str(k), str(d), str(b)]
            try:
                p = subprocess.run(cmd, capture_output=True, text=True, timeout=a.step_timeout)
            except subprocess.TimeoutExpired:
                print(f"{dtype} k={k} d={d} b={b}: no result within {a.step_timeout} s; stopping", file=sys.stderr)
                return 1
            line = [x for x in p.stdout.splitlines() if x.startswith("RESULT ")]
            if p.returncode != 0 or not line:
                print(f"{dtype} k={k} d={d} b={b}: exit {p.returncode}\n{p.stdout}\n{p.stderr}; stopping", file=sys.stderr)
                return 1
            rows.append(json.loads(line[-1][len("RESULT "):]))
            print(json.dumps(rows[-1]), flush=True)
    doc = {"what": "general-smoothness Matern: forward launch, slab backward without / with grad_nu, closed-form slab backward "
                   "(Matern-3/2) on the same inputs; HIP events, median of 5 alternating rounds after a warm-up",
           "tool": "tools/genbwdbench.py", "rows": rows}
    if a.lds:
        doc = {"what": "general-smoothness Matern: forward launch, slab backward and LDS workgroup backward without / with grad_nu, "
                       "LDS backward with every cotangent, same inputs, same process; HIP events, median / min / max of 3 "
                       "alternating rounds after a warm-up",
               "tool": "tools/genbwdbench.py --lds", "rows": rows}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
