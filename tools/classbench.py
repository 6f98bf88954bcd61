#!/usr/bin/env python3
"""What the classification path costs, on seeded Gaussian mixtures (2 and 10 classes) at the two headline shapes
(k = 30, d = 40 fp32 and k = 50, d = 8 fp64), 1 M test rows against a 1 M-row training table:

  (a) ``classify_any`` with the label partition (k-NN -> mgp_class_partition -> fused posterior on the non-constant
      neighbourhoods -> mgp_class_scatter) against the same call with EVERY neighbourhood solved, next to the measured
      non-constant share.  The neighbour lists are computed once and handed to both through a fixed lookup: the
      k-NN scan is the same work in both and is reported on its own.
  (b) one cross-entropy objective evaluation through the functor layer (fused posterior + mgp_class_sums) against
      the fused posterior launch alone -- what the sums kernel adds.
  (c) L-BFGS-B on the cross-entropy with the analytic gradient against finite differences: objective evaluations
      (fused forward launches) and seconds to the optimum, and the two optima.

Every timed call is warmed up once; times are the mean of ``--reps`` calls between device synchronisations.  Prints
one JSON line per shape; ``--out`` also writes them as a JSON list.

    python tools/classbench.py --out profiles/classify_bench.json
"""

import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import numpy as np  # noqa: E402
import torch  # noqa: E402


class FixedLookup:
    def __init__(self, indices):
        self.indices = indices

    def get_nns(self, test):
        return self.indices, None


def model(ls):
    from muygpys_amd.gp import MuyGPS
    from muygpys_amd.gp.deformation import Isotropy, l2
    from muygpys_amd.gp.hyperparameter import FixedScale, Parameter
    from muygpys_amd.gp.kernels import Matern
    from muygpys_amd.gp.noise import HomoscedasticNoise

    return MuyGPS(kernel=Matern(smoothness=Parameter(1.5), deformation=Isotropy(l2, length_scale=Parameter(ls, (0.2, 50.0)))),
                  noise=HomoscedasticNoise(1e-3), scale=FixedScale())


def timed(fn, reps):
    fn()  # warm-up (first-use allocations, prepared tables)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--b", type=int, default=1_000_000)
    ap.add_argument("--b-objective", type=int, default=200_000)
    ap.add_argument("--b-optimise", type=int, default=20_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-optimise", action="store_true")
    args = ap.parse_args()
    from muygpys_amd import fused as F
    from muygpys_amd.examples import classify as Cl
    from muygpys_amd.neighbors import NN_Wrapper
    from muygpys_amd.optimize import L_BFGS_B_optimize
    from muygpys_amd.optimize.loss import cross_entropy_fn

    dev = torch.device("cuda:0")
    rows = []
    for dt, k, d, sep in ((torch.float32, 30, 40, 0.45), (torch.float64, 50, 8, 1.0)):
        for classes in (2, 10):
            gen = torch.Generator(device=dev).manual_seed(1000 * classes + d)
            centres = torch.randn((classes, d), device=dev, dtype=dt, generator=gen) * sep
            ids = torch.randint(0, classes, (args.n,), device=dev, generator=gen)
            X = centres[ids] + torch.randn((args.n, d), device=dev, dtype=dt, generator=gen)
            tid = torch.randint(0, classes, (args.b,), device=dev, generator=gen)
            Xt = centres[tid] + torch.randn((args.b, d), device=dev, dtype=dt, generator=gen)
            Y = -torch.ones((args.n, classes), device=dev, dtype=dt)
            Y[torch.arange(args.n, device=dev), ids] = 1.0
            ls = float(np.sqrt(d))
            m = model(ls)
            rec = dict(dtype=str(dt).split(".")[-1], k=k, d=d, classes=classes, n=args.n, b=args.b, reps=args.reps)
            nbrs = NN_Wrapper(X, k)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            nn = nbrs.get_nns(Xt)[0]
            torch.cuda.synchronize()
            rec["knn_ms"] = (time.perf_counter() - t0) * 1e3
            look = FixedLookup(nn)
            # (a)
            pred, _, nonconstant, _ = Cl._partition_and_solve(m, Xt, X, look, Y, False)
            rec["nonconstant_share"] = float(nonconstant.double().mean())
            rec["accuracy"] = float((pred.argmax(dim=1) == tid).double().mean())
            rec["classify_partition_ms"] = timed(lambda: Cl._partition_and_solve(m, Xt, X, look, Y, False), args.reps)
            rec["classify_all_solved_ms"] = timed(lambda: Cl._partition_and_solve(m, Xt, X, look, Y, False, partition=False), args.reps)
            rec["partition_speedup"] = rec["classify_all_solved_ms"] / rec["classify_partition_ms"]
            # (b)
            bo = min(args.b_objective, args.n)
            bi = torch.randperm(args.n, device=dev, generator=gen)[:bo].sort().values
            bni = nbrs.get_batch_nns(bi)[0]
            cross, pair, y_b, y_nn = m.make_train_tensors(bi, bni, X, Y)
            obj = L_BFGS_B_optimize.make_obj_fn(m, y_b, y_nn, cross, pair, loss_fn=cross_entropy_fn)
            spec = F.KernelSpec("matern15", "l2", ls, 1e-3)
            rec["b_objective"] = bo
            rec["objective_ms"] = timed(lambda: obj(length_scale=ls), args.reps)
            rec["fused_alone_ms"] = timed(lambda: F.posterior_mean_var(spec, X, X, bi, bni, Y, want_ykinvy=True), args.reps)
            mean = F.posterior_mean_var(spec, X, X, bi, bni, Y)[0]
            rec["class_sums_ms"] = timed(lambda: cross_entropy_fn(mean, y_b), args.reps)
            # (c)
            if not args.skip_optimise:
                bo2 = min(args.b_optimise, bo)
                bi2, bni2 = bi[:bo2], bni[:bo2]
                calls = {"n": 0}
                real = F.posterior_mean_var

                def counted(*a, **kw):
                    calls["n"] += 1
                    return real(*a, **kw)

                F.posterior_mean_var = counted
                try:
                    for analytic in (False, True):
                        mm = model(1.0)
                        cr, pr, yb2, ynn2 = mm.make_train_tensors(bi2, bni2, X, Y)
                        calls["n"] = 0
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        new = L_BFGS_B_optimize(mm, yb2, ynn2, cr, pr, loss_fn=cross_entropy_fn, analytic_gradient=analytic)
                        torch.cuda.synchronize()
                        tag = "analytic" if analytic else "finite_difference"
                        rec[f"lbfgs_{tag}_s"] = time.perf_counter() - t0
                        rec[f"lbfgs_{tag}_evaluations"] = calls["n"]
                        rec[f"lbfgs_{tag}_length_scale"] = float(new.kernel.deformation.length_scale())
                finally:
                    F.posterior_mean_var = real
                rec["b_optimise"] = bo2
            print(json.dumps(rec), flush=True)
            rows.append(rec)
            del X, Xt, Y, nn, nbrs, look, cross, pair, y_nn, obj
            F.clear_caches()
            torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
