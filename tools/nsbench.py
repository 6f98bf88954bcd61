#!/usr/bin/env python3
"""A length scale per neighbourhood: what the NS launch costs (GPU; writes profiles/nonstationary_bench.json).

Three comparisons per shape, the two sides of each alternating in one process (round-robin over ``--rounds`` rounds of
``--reps`` timed calls between device events, after a warm-up of every side):

  ns_vs_scalar        mgp_posterior_ns_{generic,large}_* against the scalar launch of the same family by name
                      (path="generic" / "large"), with the spread of the scalar launch's own rounds next to the ratio
  ns_vs_materialised  the NS launch against the per-function kernels with the scale broadcast along axis 0
                      (distances -> / l_i -> kernel -> nugget -> mgp_solve_*), at a batch that fits memory
  wave_gap            (k = 30, d = 40, fp32 alone) the dispatcher's scalar launch -- the wave kernel a stationary model
                      gets -- against the NS launch: what a nonstationary model gives up on the workgroup kernel

    python tools/nsbench.py [--quick] [--out profiles/nonstationary_bench.json]
"""

import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from muygpys_amd import _lib  # noqa: E402
from muygpys_amd.fused import KernelSpec, posterior_mean_var  # noqa: E402

SHAPES = [  # (dtype, k, d, neighbourhoods, family)
    ("float32", 30, 40, 200_000, "generic"),
    ("float64", 50, 8, 200_000, "generic"),
    ("float32", 100, 40, 200_000, "generic"),
    ("float32", 300, 8, 20_000, "large"),
]


def timed(fn, reps):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / reps  # ms per call


def alternate(sides, rounds, reps):
    """{name: [ms per call, one entry per round]}; every side warmed first, then round-robin."""
    for fn in sides.values():
        fn()
    torch.cuda.synchronize()
    out = {name: [] for name in sides}
    for _ in range(rounds):
        for name, fn in sides.items():
            out[name].append(timed(fn, reps))
    return out


def summary(ms):
    a = np.asarray(ms)
    return dict(median_ms=float(np.median(a)), min_ms=float(a.min()), max_ms=float(a.max()),
                spread=float((a.max() - a.min()) / np.median(a)))


def materialised(spec_kernel, metric, X, bi, ni, y, ls, noise):
    from muygpys_amd._src.gp.kernels import hip as K
    from muygpys_amd._src.gp.muygps import hip as M
    from muygpys_amd._src.gp.noise import hip as N
    from muygpys_amd._src.gp.tensors import hip as T

    p = 1 if metric == "l2" else 2
    pair = T._pairwise_distances(X, ni, metric) / ls[:, None, None] ** p
    cross = T._crosswise_distances(X, X, bi, ni, metric) / ls[:, None] ** p
    Kin = N._homoscedastic_perturb(K._apply(pair, spec_kernel, 1.0), noise)
    Kc = K._apply(cross, spec_kernel, 1.0)
    return M._solve(Kin, Kc, y[ni], want=("mean", "var"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="a tenth of the neighbourhoods, fewer rounds (rehearsal)")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles",
                                                  "nonstationary_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("nsbench needs a ROCm device: nothing is measured without one")
    dev = torch.device("cuda:0")
    rounds, reps = (3, 2) if a.quick else (a.rounds, a.reps)
    results = []
    for dtype, k, d, b, family in SHAPES:
        b = b // 10 if a.quick else b
        dt = getattr(torch, dtype)
        rng = np.random.default_rng(k * 1000 + d)
        n = max(4 * k, 20_000)
        X = torch.as_tensor(rng.uniform(size=(n, d)) * 3.0 / np.sqrt(d / 6.0), device=dev, dtype=dt)
        y = torch.as_tensor(rng.normal(size=n), device=dev, dtype=dt)
        bi = torch.as_tensor(rng.integers(0, n, size=b), device=dev)
        ni = torch.as_tensor(rng.integers(0, n, size=(b, k)), device=dev)
        ls = torch.as_tensor(np.exp(rng.uniform(np.log(1.0), np.log(5.0), size=b)), device=dev, dtype=dt)
        scalar = KernelSpec("matern15", "l2", 3.0, 0.05)
        ns = KernelSpec("matern15", "l2", 1.0, 0.05, length_scale_batch=ls)
        mean, var = torch.empty((b, 1), device=dev, dtype=dt), torch.empty(b, device=dev, dtype=dt)
        kw = dict(out_mean=mean, out_var=var, packed=False)
        info = torch.zeros(1, device=dev, dtype=torch.int32)  # (the caller's own counter: no host read per call)
        names = {}

        def run(spec, path, tag, **more):
            def fn():
                posterior_mean_var(spec, X, X, bi, ni, y, path=path, info=info, **kw, **more)
                names[tag] = _lib.last_kernel()
            return fn

        rec = dict(dtype=dtype, k=k, d=d, neighbourhoods=b, family=family, rounds=rounds, reps=reps)
        t = alternate({"scalar": run(scalar, family, "scalar"), "ns": run(ns, family, "ns")}, rounds, reps)
        rec["ns_vs_scalar"] = dict(scalar=summary(t["scalar"]), ns=summary(t["ns"]), kernels=dict(names),
                                   ratio=float(np.median(t["ns"]) / np.median(t["scalar"])),
                                   scalar_spread=summary(t["scalar"])["spread"])
        mb = min(b, max(256, int(2e9 // (k * k * X.element_size() * 4))))  # (the (b, k, k) tensors of the route fit)
        bi_m, ni_m, ls_m = bi[:mb].contiguous(), ni[:mb].contiguous(), ls[:mb].contiguous()
        ns_m = KernelSpec("matern15", "l2", 1.0, 0.05, length_scale_batch=ls_m)
        sides = {"ns": lambda: posterior_mean_var(ns_m, X, X, bi_m, ni_m, y, path=family, info=info, packed=False),
                 "materialised": lambda: materialised("matern15", "l2", X, bi_m, ni_m, y, ls_m, 0.05)}
        t = alternate(sides, rounds, reps)
        rec["ns_vs_materialised"] = dict(neighbourhoods=mb, ns=summary(t["ns"]), materialised=summary(t["materialised"]),
                                         speedup=float(np.median(t["materialised"]) / np.median(t["ns"])))
        if (dtype, k, d) == ("float32", 30, 40):
            t = alternate({"dispatcher": run(scalar, "auto", "dispatcher"), "ns": run(ns, family, "ns")}, rounds, reps)
            rec["wave_gap"] = dict(dispatcher=summary(t["dispatcher"]), ns=summary(t["ns"]), kernels=dict(names),
                                   ratio=float(np.median(t["ns"]) / np.median(t["dispatcher"])))
        assert int(info.item()) == 0, "a neighbourhood did not factorise: the timings are not of the intended work"
        print(json.dumps(rec), flush=True)
        results.append(rec)
    out = dict(device=torch.cuda.get_device_name(0), tool="tools/nsbench.py", quick=bool(a.quick), shapes=results)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
