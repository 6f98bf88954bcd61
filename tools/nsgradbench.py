#!/usr/bin/env python3
"""A length scale per neighbourhood: what the analytic gradient costs (GPU; writes
profiles/nonstationary_backward_bench.json).  The protocol of tools/nsbench.py: the two sides of a comparison alternate
in one process, rounds of timed calls between device events after a warm-up of every side, medians, and the run-to-run
spread of the scalar side next to every ratio.

  backward_ns_vs_scalar  one NS hyper-parameter backward launch (mgp_hyper_backward_ns_* / _ns_large_*, LOOCV form)
                         against the scalar launch the same call makes without length_scale_batch (MGP_BACKWARD_LDS
                         unset: the scalar side is whatever its ladder picks; both kernel names are recorded)
  gradient_vs_forwards   (the first two shapes) one analytic gradient evaluation -- fused.loocv_value_and_grad on the NS
                         kernels plus the pullback to the knots -- against p + 1 evaluations of the knot GP and the NS
                         forward, p the knot count of examples/nonstationary_regression.py

    python tools/nsgradbench.py [--quick] [--out profiles/nonstationary_backward_bench.json]

``--forward wave`` times one analytic gradient evaluation under ``fused.ns_forward("wave")`` next to the default route's
instead (``forward_wave_main``) -> the "gradient" records of profiles/nonstationary_wave_bench.json.
"""

import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from muygpys_amd import _lib, fused  # noqa: E402
from muygpys_amd.fused import KernelSpec  # noqa: E402
from tools.nsbench import SHAPES, alternate, summary  # noqa: E402

KNOTS = 4  # (examples/nonstationary_regression.py: knot_count)


def hierarchical(d, knots, rng):
    from muygpys_amd.gp.deformation import Isotropy, l2
    from muygpys_amd.gp.hyperparameter import Parameter, VectorParameter
    from muygpys_amd.gp.hyperparameter.experimental import HierarchicalParameter
    from muygpys_amd.gp.kernels import RBF

    values = VectorParameter(*[Parameter(3.0, (1.0, 5.0)) for _ in range(knots)])
    higher = RBF(deformation=Isotropy(l2, length_scale=Parameter(3.0)))
    raw = HierarchicalParameter(rng.uniform(size=(knots, d)) * 3.0 / np.sqrt(d / 6.0), values, higher)
    return Isotropy(l2, length_scale=raw).length_scale


def forward_wave_main(a, dev, rounds, reps):
    """--forward wave: one analytic knot-gradient evaluation (gradient_vs_forwards' `analytic`) under
    fused.ns_forward("wave") and under the default mode, alternating, at the first two shapes -> the "gradient" records of
    profiles/nonstationary_wave_bench.json (tools/nsbench.py --wave writes the rest of that file and keeps these)."""
    from tools.nsbench import WAVE_OUT

    records = []
    for dtype, k, d, b, _ in SHAPES[:2]:
        b = b // 10 if a.quick else b
        dt = getattr(torch, dtype)
        rng = np.random.default_rng(k * 1000 + d)
        n = max(4 * k, 20_000)
        X = torch.as_tensor(rng.uniform(size=(n, d)) * 3.0 / np.sqrt(d / 6.0), device=dev, dtype=dt)
        y = torch.as_tensor(rng.normal(size=n), device=dev, dtype=dt)
        bi = torch.as_tensor(rng.integers(0, n, size=b), device=dev)
        ni = torch.as_tensor(rng.integers(0, n, size=(b, k)), device=dev)
        hp, bf, trial = hierarchical(d, KNOTS, rng), X[bi].contiguous(), [0]

        def analytic(mode):
            def fn():
                trial[0] += 1  # (a new trial point every evaluation: nothing comes out of the parameter's caches)
                knots = {f"length_scale{j}": 3.0 + 1e-3 * ((trial[0] + j) % 97) for j in range(KNOTS)}
                spec = KernelSpec("matern15", "l2", 1.0, 0.05, length_scale_batch=hp(bf, **knots))
                with fused.ns_forward(mode):
                    _, g_l, _ = fused.loocv_value_and_grad(spec, X, y, bi, ni, packed=False)
                hp.pullback(bf, g_l)
            return fn

        t = alternate({"workgroup": analytic("workgroup"), "wave": analytic("wave")}, rounds, reps)
        rec = dict(dtype=dtype, k=k, d=d, neighbourhoods=b, knots=KNOTS, rounds=rounds, reps=reps,
                   workgroup=summary(t["workgroup"]), wave=summary(t["wave"]),
                   speedup=float(np.median(t["workgroup"]) / np.median(t["wave"])))
        print(json.dumps(rec), flush=True)
        records.append(rec)
    out = dict(device=torch.cuda.get_device_name(0), tool="tools/nsbench.py --wave", shapes=[])
    if os.path.exists(WAVE_OUT):
        with open(WAVE_OUT) as f:
            out = json.load(f)
    out["gradient"] = records
    out["gradient_tool"] = "tools/nsgradbench.py --forward wave"
    with open(WAVE_OUT, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", WAVE_OUT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="a tenth of the neighbourhoods, fewer rounds (rehearsal)")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles",
                                                  "nonstationary_backward_bench.json"))
    ap.add_argument("--forward", choices=fused.NS_FORWARD_MODES, default="workgroup",
                    help="wave: one analytic gradient evaluation under fused.ns_forward('wave') next to the default route's")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("nsgradbench needs a ROCm device: nothing is measured without one")
    dev = torch.device("cuda:0")
    rounds, reps = (3, 2) if a.quick else (a.rounds, a.reps)
    if a.forward == "wave":
        return forward_wave_main(a, dev, rounds, reps)
    results = []
    for at, (dtype, k, d, b, _) in enumerate(SHAPES):
        b = b // 10 if a.quick else b
        dt = getattr(torch, dtype)
        rng = np.random.default_rng(k * 1000 + d)
        n = max(4 * k, 20_000)
        X = torch.as_tensor(rng.uniform(size=(n, d)) * 3.0 / np.sqrt(d / 6.0), device=dev, dtype=dt)
        y = torch.as_tensor(rng.normal(size=n), device=dev, dtype=dt)
        bi = torch.as_tensor(rng.integers(0, n, size=b), device=dev)
        ni = torch.as_tensor(rng.integers(0, n, size=(b, k)), device=dev)
        ls = torch.as_tensor(np.exp(rng.uniform(np.log(1.0), np.log(5.0), size=b)), device=dev, dtype=dt)
        specs = {"scalar": KernelSpec("matern15", "l2", 3.0, 0.05),
                 "ns": KernelSpec("matern15", "l2", 1.0, 0.05, length_scale_batch=ls)}
        gm, gv, gyk = (torch.as_tensor(rng.normal(size=b), device=dev, dtype=dt) for _ in range(3))
        info = torch.zeros(1, device=dev, dtype=torch.int32)
        names = {}

        def backward(tag):
            inp = fused._normalize(specs[tag], X, X, bi, ni, y, responses="single", per_neighbourhood=tag == "ns")

            def fn():
                fused._hyper_partials(specs[tag], inp, info, gm, gv, gyk)
                names[tag] = _lib.last_kernel()
            return fn

        rec = dict(dtype=dtype, k=k, d=d, neighbourhoods=b, rounds=rounds, reps=reps)
        t = alternate({"scalar": backward("scalar"), "ns": backward("ns")}, rounds, reps)
        rec["backward_ns_vs_scalar"] = dict(scalar=summary(t["scalar"]), ns=summary(t["ns"]), kernels=dict(names),
                                            ratio=float(np.median(t["ns"]) / np.median(t["scalar"])),
                                            scalar_spread=summary(t["scalar"])["spread"])
        if at < 2:
            hp = hierarchical(d, KNOTS, rng)
            bf = X[bi].contiguous()
            trial = [0]

            def knot_values():  # (a new trial point every evaluation: nothing comes out of the parameter's caches)
                trial[0] += 1
                return {f"length_scale{j}": 3.0 + 1e-3 * ((trial[0] + j) % 97) for j in range(KNOTS)}

            def analytic():
                spec = KernelSpec("matern15", "l2", 1.0, 0.05, length_scale_batch=hp(bf, **knot_values()))
                _, g_l, _ = fused.loocv_value_and_grad(spec, X, y, bi, ni, packed=False)
                hp.pullback(bf, g_l)

            def forwards():
                for _ in range(KNOTS + 1):
                    spec = KernelSpec("matern15", "l2", 1.0, 0.05, length_scale_batch=hp(bf, **knot_values()))
                    fused._loocv_forward(spec, X, y, bi, ni, False, 1.5)[0].tolist()  # (the objective's host read)

            t = alternate({"forwards": forwards, "analytic": analytic}, rounds, reps)
            one_forward = float(np.median(t["forwards"])) / (KNOTS + 1)
            rec["gradient_vs_forwards"] = dict(
                knots=KNOTS, forwards=summary(t["forwards"]), analytic=summary(t["analytic"]),
                speedup=float(np.median(t["forwards"]) / np.median(t["analytic"])),
                break_even_knots=float(np.median(t["analytic"]) / one_forward - 1.0))
        print(json.dumps(rec), flush=True)
        results.append(rec)
    out = dict(device=torch.cuda.get_device_name(0), tool="tools/nsgradbench.py", quick=bool(a.quick), shapes=results)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
