#!/usr/bin/env python3
"""Neighbourhoods per second of the shear posterior (mean (b, 3) + covariance (b, 3, 3)) by three routes:

  fused          MuyGPS on lazy tensors: one mgp_shear_posterior_* launch per evaluation
  materialised   MuyGPS on materialised tensors: shear tensor kernels, block nugget, mgp_solve_multi_* (mean and
                 covariance each factorise)
  numpy (fp64)   the tests' numpy statement (tests/shear_oracle.py, linalg.solve) with the BLAS pools limited to ONE
                 thread (threadpoolctl), in float64 whatever the GPU rows' dtype: one figure per k and model, repeated
                 in both dtype rows

for fp32 / fp64, k in {20, 30, 50}, ShearKernel (+ ShearNoise33) and ShearKernel2in3out (+ HomoscedasticNoise).
Every route is warmed up once before it is timed; each record carries the batch size of each route (b_fused,
b_materialised, b_numpy).  Neighbourhoods are k distinct random rows of a 100 k-point table (the cost does not depend
on the values).  Prints one JSON line per shape; ``--out`` also writes them as a JSON list.

    python tools/shearbench.py --out profiles/shear_bench.json
"""

import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def model(kind, ell, eps):
    from muygpys_amd.gp.deformation import F2, DifferenceIsotropy
    from muygpys_amd.gp.hyperparameter import FixedScale, ScalarParam
    from muygpys_amd.gp.kernels import ShearKernel, ShearKernel2in3out
    from muygpys_amd.gp.muygps import MuyGPS
    from muygpys_amd.gp.noise import HomoscedasticNoise, ShearNoise33

    dfm = DifferenceIsotropy(F2, length_scale=ScalarParam(ell))
    if kind == "33":
        return MuyGPS(kernel=ShearKernel(deformation=dfm), noise=ShearNoise33(eps), scale=FixedScale())
    return MuyGPS(kernel=ShearKernel2in3out(deformation=dfm), noise=HomoscedasticNoise(eps), scale=FixedScale())


def gpu_rate(fn, b, reps):
    fn()  # warm-up (and first-use allocations)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return b * reps / (time.perf_counter() - t0)


def numpy_one_thread(fn, b):
    """(neighbourhoods/s of ``fn``, warmed up once, with every BLAS / OpenMP pool of the process limited to one thread;
    the largest pool size seen inside the limit -- 1 when it held)."""
    from threadpoolctl import threadpool_info, threadpool_limits

    with threadpool_limits(limits=1):
        threads = max([p["num_threads"] for p in threadpool_info()] or [1])
        fn(4)  # warm-up
        t0 = time.perf_counter()
        fn(b)
        return b / (time.perf_counter() - t0), threads


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--n", type=int, default=100_000)
    ap.add_argument("--b-fused", type=int, default=200_000)
    ap.add_argument("--b-mat", type=int, default=20_000)
    ap.add_argument("--b-numpy", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ks", default="20,30,50")
    ap.add_argument("--only-fused", action="store_true")
    args = ap.parse_args()
    from tests import shear_oracle as O

    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    ell, eps = 1e-3, 1e-2
    Xh, Yh = rng.uniform(size=(args.n, 2)), rng.normal(size=(args.n, 3))
    numpy_rate = {}
    rows = []
    for dt in (torch.float32, torch.float64):
        X, Y3 = torch.tensor(Xh, device=dev, dtype=dt), torch.tensor(Yh, device=dev, dtype=dt)
        for k in (int(v) for v in args.ks.split(",")):
            for kind in ("33", "23"):
                m = model(kind, ell, eps)
                # the response table holds the observed components: all three, or (gamma1, gamma2)
                Y = Y3 if kind == "33" else Y3[:, 1:].contiguous()
                rec = dict(dtype=str(dt).split(".")[-1], k=k, model="ShearKernel" if kind == "33" else "ShearKernel2in3out")

                def run(b, materialize):
                    bi = torch.randint(0, args.n, (b,), device=dev)
                    # k distinct random rows per neighbourhood (a repeated row makes the system singular up to eps)
                    ni = (torch.randint(0, args.n, (b, 1), device=dev) + torch.arange(k, device=dev) * (args.n // k)) % args.n

                    def once():
                        cr, pr, nt = m.make_predict_tensors(bi, ni, X, X, Y, materialize=materialize)
                        nt = nt.swapaxes(-2, -1)
                        Kin, Kc = m.kernel(pr), m.kernel(cr)
                        m.posterior_mean(Kin, Kc, nt)
                        m.posterior_variance(Kin, Kc)

                    return once

                rec["b_fused"] = args.b_fused
                rec["fused"] = gpu_rate(run(args.b_fused, False), args.b_fused, args.reps)
                if not args.only_fused:
                    rec["b_materialised"] = args.b_mat
                    rec["materialised"] = gpu_rate(run(args.b_mat, True), args.b_mat, args.reps)
                    rec["fused_over_materialised"] = rec["fused"] / rec["materialised"]
                    if (k, kind) not in numpy_rate:
                        noise = "shear33" if kind == "33" else "homoscedastic"
                        bi = rng.integers(0, args.n, args.b_numpy)
                        ni = (rng.integers(0, args.n, (args.b_numpy, 1)) + np.arange(k) * (args.n // k)) % args.n
                        numpy_rate[(k, kind)] = numpy_one_thread(
                            lambda b: O.posterior(Xh, Yh, bi[:b], ni[:b], ell, eps, kind, noise), args.b_numpy)
                    rec["b_numpy"] = args.b_numpy
                    rec["numpy_fp64_one_thread"], rec["numpy_threads"] = numpy_rate[(k, kind)]
                rec["unit"] = "neighbourhoods/s"
                print(json.dumps(rec), flush=True)
                rows.append(rec)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
