#!/usr/bin/env python3
"""The exact grid search (NN_Wrapper(..., algorithm="grid")) against the exact scan, on the GPU, at d = 2 and 3.

For every shape, batch queries over the whole table: the exact scan (the default route) timed in the same process on
the same queries, then for cell_rows in {16, 32, 64} -- and both edge rules on the clustered table -- the index build
time, the search time, the mean and the maximum of ``last_shells``, the rows scanned per query (the population of every
query's walked block, from a summed-area table of the cell counts), pair distances per second, and whether the answers
are the exact scan's on 4 000 sampled queries (entries that differ are counted, not hidden).  Times are HIP events on the
launch stream around the whole call (cells of the queries, ordering, walk, finish), after a warm-up call of the same
shape; every figure is the median of the repeats with their minimum and maximum next to it.  At 10 M x 10 M the exact
scan runs once.

Every shape runs in a fresh child process under its own time limit; the children are chained, and the first one that
fails ends the run.  Writes profiles/knn_grid_bench.json.

    python tools/knngridbench.py [--shapes d2_1m d3_1m d2_mixture d2_10m] [--repeats 3] [--out FILE]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CELL_ROWS = (16, 32, 64)
CHECK_QUERIES = 4000
# name: (table rows = batch queries, d, k, data, repeats of the exact scan (None: --repeats), time limit of the child in s)
SHAPES = {
    "d2_1m": (1_000_000, 2, 30, "uniform", None, 300),
    "d3_1m": (1_000_000, 3, 50, "uniform", None, 300),
    "d2_mixture": (1_000_000, 2, 30, "mixture", None, 300),
    "d2_10m": (10_000_000, 2, 30, "uniform", 1, 900),
}


def make_table(n, d, data, gen):
    import torch

    if data == "uniform":
        return torch.rand(n, d, generator=gen, device="cuda")
    centres = 0.1 + 0.8 * torch.rand(30, d, generator=gen, device="cuda")  # 30 clusters, sigma = 0.02
    which = torch.randint(0, 30, (n,), generator=gen, device="cuda")
    return centres[which] + 0.02 * torch.randn(n, d, generator=gen, device="cuda")


def timed(fn, repeats, warm=True):
    """(last result, {median, min, max} in ms over `repeats` calls) by HIP events on the current stream; one warm-up."""
    import torch

    if warm:
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return out, {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3),
                 "repeats": repeats, "warm_up": bool(warm)}


def rows_scanned(nn, pos, shells):
    """Per query (stored positions ``pos``): the rows of the block c_a - r .. c_a + r it walked, clipped to the grid."""
    import torch

    from muygpys_amd.neighbors import grid_cells

    g0, g1, g2 = nn.grid_shape
    counts = (nn.cell_start[1:] - nn.cell_start[:-1]).reshape(g2, g1, g0)
    sat = torch.zeros((g2 + 1, g1 + 1, g0 + 1), dtype=torch.int64, device=counts.device)
    sat[1:, 1:, 1:] = counts.cumsum(0).cumsum(1).cumsum(2)
    c = grid_cells(nn.train[pos], nn._edges).to(torch.int64)
    r = shells.to(torch.int64)[:, None]
    lo = (c - r).clamp(min=0)
    hi = torch.minimum(c + r, torch.tensor([g0 - 1, g1 - 1, g2 - 1], device=c.device)) + 1
    total = torch.zeros(len(pos), dtype=torch.int64, device=c.device)
    for s2, b2 in ((1, hi[:, 2]), (-1, lo[:, 2])):
        for s1, b1 in ((1, hi[:, 1]), (-1, lo[:, 1])):
            for s0, b0 in ((1, hi[:, 0]), (-1, lo[:, 0])):
                total += s2 * s1 * s0 * sat[b2, b1, b0]
    return total


def child(name, repeats):
    import torch

    from muygpys_amd.neighbors import NN_Wrapper

    n, d, k, data, exact_repeats, _ = SHAPES[name]
    gen = torch.Generator(device="cuda").manual_seed(20261 + len(name))
    X = make_table(n, d, data, gen)
    bi = torch.arange(n, device="cuda")
    rows = torch.randperm(n, generator=gen, device="cuda")[:CHECK_QUERIES]
    rec = {"shape": name, "table_rows": n, "queries": n, "feature_count": d, "nn_count": k, "data": data,
           "device": torch.cuda.get_device_name(0)}

    exact = NN_Wrapper(X, k)
    (want, _), rec["exact"] = timed(lambda: exact.get_batch_nns(bi), exact_repeats or repeats, warm=exact_repeats is None)
    rec["exact"]["route"] = exact.last_route
    rec["exact"]["pairs_per_s"] = round(float(n) * n / (rec["exact"]["median_ms"] * 1e-3), 1)
    want = want[rows].clone()
    del exact
    torch.cuda.empty_cache()

    rec["grid"] = []
    for edges in (("uniform", "quantile") if data == "mixture" else ("uniform",)):
        for cell_rows in CELL_ROWS:
            builds = []
            for _ in range(repeats):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                nn = NN_Wrapper(X, k, algorithm="grid", edges=edges, cell_rows=cell_rows)
                torch.cuda.synchronize()
                builds.append(1e3 * (time.perf_counter() - t0))
            (got, _), t = timed(lambda: nn.get_batch_nns(bi), repeats)
            assert nn.last_route == "grid"
            shells = nn.last_shells
            scanned = rows_scanned(nn, nn._inv[bi], shells).double()
            sizes = (nn.cell_start[1:] - nn.cell_start[:-1]).double()
            t.update(edges=edges, cell_rows=cell_rows, grid=list(nn.grid_shape),
                     build={"median_ms": round(statistics.median(builds), 3), "min_ms": round(min(builds), 3),
                            "max_ms": round(max(builds), 3), "repeats": repeats, "first_build_included": True},
                     cell_population={"mean": float(sizes.mean()), "max": int(sizes.max()), "empty": int((sizes == 0).sum())},
                     shells_mean=round(float(shells.double().mean()), 4), shells_max=int(shells.max()),
                     rows_scanned_per_query=round(float(scanned.mean()), 1), rows_scanned_max=int(scanned.max()),
                     pairs_per_s=round(float(scanned.sum()) / (t["median_ms"] * 1e-3), 1),
                     entries_differing_from_exact=int((got[rows] != want).sum()), checked_entries=int(want.numel()),
                     speedup_over_exact=round(rec["exact"]["median_ms"] / t["median_ms"], 3))
            rec["grid"].append(t)
            print(json.dumps({"shape": name, **t}), flush=True)
            del nn
            torch.cuda.empty_cache()
    print("RESULT " + json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="*", default=list(SHAPES), choices=list(SHAPES))
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "knn_grid_bench.json"))
    ap.add_argument("--child", default="", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.repeats)
    results = []
    for name in args.shapes:  # chained: a child that fails, faults or runs out of time ends the run
        cmd = ["timeout", "-k", "10", str(SHAPES[name][5]), sys.executable, os.path.abspath(__file__), "--child", name,
               "--repeats", str(args.repeats)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        sys.stdout.write(p.stdout)
        sys.stdout.flush()
        if p.returncode != 0:
            print(f"[knngridbench] {name}: exit status {p.returncode}; nothing further is started", file=sys.stderr)
            break
        results += [json.loads(ln[7:]) for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"tool": "tools/knngridbench.py", "cell_rows": CELL_ROWS, "shapes": results}, f, indent=1)
        f.write("\n")
    return 0 if len(results) == len(args.shapes) else 1


if __name__ == "__main__":
    sys.exit(main())
