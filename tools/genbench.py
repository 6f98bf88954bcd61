#!/usr/bin/env python3
"""General-smoothness Matern on the fused path, fp32 and fp64, against the fixed nu = 3/2 closed form (GPU box):
python tools/genbench.py  -> one JSON line (ms per launch, M neighbourhoods/s, kernel that served the call)."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from muygpys_amd import _lib
from muygpys_amd.fused import KernelSpec, posterior_mean_var


def main():
    out = {}
    gen = torch.Generator(device="cuda").manual_seed(5)
    for dtype, (N, d, k, b) in (("f32", (400_000, 40, 30, 400_000)), ("f64", (400_000, 40, 30, 200_000)),
                                ("f64_k10_d6", (300_000, 6, 10, 300_000))):
        td = torch.float32 if dtype == "f32" else torch.float64
        X = torch.randn(N, d, device="cuda", generator=gen).to(td)
        y = torch.randn(N, device="cuda", generator=gen).to(td)
        bi = torch.arange(b, device="cuda")
        ni = torch.randint(0, N - 1, (b, k), device="cuda", generator=gen)
        ni = ni + (ni >= bi[:, None])
        ell = float(np.sqrt(d / 40.0) * 6.0)
        res = {}
        for name, spec in (("fixed_nu_1.5", KernelSpec("matern15", "l2", ell, 1e-3)),
                           ("free_nu_1.5", KernelSpec("matern_gen", "l2", ell, 1e-3, smoothness=1.5)),
                           ("free_nu_0.8", KernelSpec("matern_gen", "l2", ell, 1e-3, smoothness=0.8)),
                           ("free_nu_4.2", KernelSpec("matern_gen", "l2", ell, 1e-3, smoothness=4.2))):
            ts = []
            for r in range(7):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                m, v = posterior_mean_var(spec, X, X, bi, ni, y, packed=True)
                e1.record()
                torch.cuda.synchronize()
                ts.append(e0.elapsed_time(e1))
            ms = float(np.median(ts[2:]))
            res[name] = {"ms": ms, "M_nbhd_per_s": b / ms / 1e3, "kernel": _lib.last_kernel(), "finite": bool(torch.isfinite(m).all())}
        out[dtype] = {"points": N, "d": d, "k": k, "batch": b, **res}
    print(json.dumps(out))


# ---- beyond 64 slots: the fused launch of a workgroup kernel against the materialising route ---------------------------
BEYOND64_SHAPES = ((100, 40, 200_000), (300, 8, 20_000))  # (nn_count, features, batch)
BEYOND64_NUS = (0.8, 2.2)


def _timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def beyond64(out_path, rounds=3):
    """Per shape, float width and smoothness: one fused launch (mgp_posterior_gen_* / mgp_posterior_gen_large_*) against
    the route a caller materialises through when the fused path refuses -- mgp_pairwise_dists_* + mgp_crosswise_dists_*,
    mgp_matern_gen_* on both, mgp_perturb_*, mgp_solve_* / mgp_solve_large_* -- in one process, alternating after a
    warm-up of each, device events around each; and the closed-form nu = 3/2 launch of the same kernel family as the
    floor.  Every buffer of the materialising route is allocated outside the timed region (its best case)."""
    P, lib = _lib.ptr, _lib.load()
    gen = torch.Generator(device="cuda").manual_seed(5)
    N, eps = 400_000, 1e-3
    results = []
    for k, d, b in BEYOND64_SHAPES:
        for dtype in ("f32", "f64"):
            td = torch.float32 if dtype == "f32" else torch.float64
            X = torch.randn(N, d, device="cuda", generator=gen).to(td)
            y = torch.randn(N, device="cuda", generator=gen).to(td)
            bi = torch.arange(b, device="cuda")
            ni = torch.randint(0, N - 1, (b, k), device="cuda", generator=gen)
            ni = ni + (ni >= bi[:, None])
            ell = float(np.sqrt(d / 40.0) * 6.0)
            family = "generic" if k <= lib.mgp_max_nn_count_gen(X.element_size(), 1) else "large"
            # the materialising route's tensors: distances, covariances, the perturbed matrix, gathered responses
            pd, Kin, Kp = (torch.empty((b, k, k), device="cuda", dtype=td) for _ in range(3))
            cd, Kc = (torch.empty((b, k), device="cuda", dtype=td) for _ in range(2))
            mean, var = torch.empty((b, 1), device="cuda", dtype=td), torch.empty(b, device="cuda", dtype=td)
            info = torch.zeros(1, device="cuda", dtype=torch.int32)
            ws = _lib.large_workspace(td, k, 1, b, X.device) if family == "large" else None
            st = _lib.stream_ptr()

            def materialised(nu):
                rcs = [_lib.fn("pairwise_dists", td)(P(X), d, P(ni), b, k, 0, P(pd), st),
                       _lib.fn("crosswise_dists", td)(P(X), P(X), d, P(bi), P(ni), b, k, 0, P(cd), st),
                       _lib.fn("matern_gen", td)(P(pd), pd.numel(), 1.0 / ell, nu, P(Kin), st),
                       _lib.fn("matern_gen", td)(P(cd), cd.numel(), 1.0 / ell, nu, P(Kc), st),
                       _lib.fn("perturb", td)(P(Kin), b, k, _lib.NOISE_SCALAR, eps, None, P(Kp), st)]
                Yn = y[ni].reshape(b, k, 1)  # (the gather of the responses belongs to the route)
                if family == "large":
                    rcs.append(_lib.fn("solve_large", td)(P(Kp), P(Kc), P(Yn), b, k, 1, 1.0, P(mean), P(var), None, None, P(info),
                                                          P(ws), ws.numel(), st))
                else:
                    rcs.append(_lib.fn("solve", td)(P(Kp), P(Kc), P(Yn), b, k, 1, 1.0, P(mean), P(var), None, None, P(info), st))
                assert not any(rcs), rcs

            floor_spec = KernelSpec("matern15", "l2", ell, eps)
            posterior_mean_var(floor_spec, X, X, bi, ni, y, path=family, packed=False)
            floor = float(np.median([_timed(lambda: posterior_mean_var(floor_spec, X, X, bi, ni, y, path=family, packed=False))
                                     for _ in range(rounds)]))
            floor_kernel = _lib.last_kernel()
            for nu in BEYOND64_NUS:
                spec = KernelSpec("matern_gen", "l2", ell, eps, smoothness=nu)
                got = {}

                def fused_launch():
                    got["mv"] = posterior_mean_var(spec, X, X, bi, ni, y)

                fused_launch()
                kernel = _lib.last_kernel()
                materialised(nu)
                torch.cuda.synchronize()
                agree = float(((got["mv"][0] - mean[:, 0]).abs().max() / mean.abs().max()).item())
                tf, tm = [], []
                for _ in range(rounds):
                    tf.append(_timed(fused_launch))
                    tm.append(_timed(lambda: materialised(nu)))
                row = {"k": k, "d": d, "batch": b, "dtype": dtype, "nu": nu, "kernel": kernel, "fused_ms": float(np.median(tf)),
                       "materialised_ms": float(np.median(tm)), "closed_form_nu_1.5_ms": floor, "closed_form_kernel": floor_kernel,
                       "materialised_tensor_GB": (3 * pd.numel() + 2 * cd.numel()) * pd.element_size() / 1e9,
                       "max_mean_difference_rel": agree}
                row["materialised_over_fused"] = row["materialised_ms"] / row["fused_ms"]
                results.append(row)
                print(json.dumps(row), flush=True)
            del pd, Kin, Kp, cd, Kc, X, y, ni, ws
            torch.cuda.empty_cache()
    with open(out_path, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "points": N, "rounds": rounds, "results": results}, f, indent=1)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--beyond64":
        default = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "gen_beyond64_bench.json")
        beyond64(sys.argv[2] if len(sys.argv) > 2 else default)
    else:
        main()
