#!/usr/bin/env python3
"""The inverted-cell index (nn_method="ivf") against the exact scan, on the GPU: recall / time frontier per shape.

For every shape: index build time, and for nprobe in {4, 8, 16, 32, 64} the time of the batch query, recall@k against
nn_method="exact" on 4 000 sampled queries and the number of queries that fell back to the exact path
(``last_short.sum()``); the exact scan is timed in the same process on the same queries.  Times are HIP events on the
launch stream around the whole call (probe selection, scan, finish, fallback), after a warm-up call of the same shape;
every figure is the median of the repeats with their minimum and maximum next to it.

Every shape runs in a fresh child process under its own time limit; the children are chained, and the first one that
fails ends the run.  Writes profiles/knn_ivf_bench.json.

    python tools/ivfbench.py [--shapes d8_1m d8_10m d40_mixture d40_gaussian] [--repeats 3] [--out FILE]
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

NPROBES = (4, 8, 16, 32, 64)
RECALL_QUERIES = 4000
# name: (table rows, batch queries, d, k, data, time limit of the child in seconds)
SHAPES = {
    "d8_1m": (1_000_000, 1_000_000, 8, 50, "gaussian", 420),
    "d8_10m": (10_000_000, 2_000_000, 8, 50, "gaussian", 600),
    "d40_mixture": (1_000_000, 1_000_000, 40, 30, "mixture", 420),
    "d40_gaussian": (1_000_000, 1_000_000, 40, 30, "gaussian", 420),
}


def make_table(n, d, data, gen):
    import torch

    if data == "gaussian":
        return torch.randn(n, d, generator=gen, device="cuda")
    # 30 clusters, four principal directions each: low intrinsic dimension at any d
    centres = 4.0 * torch.randn(30, d, generator=gen, device="cuda")
    basis = torch.randn(30, 4, d, generator=gen, device="cuda") / 2.0
    which = torch.randint(0, 30, (n,), generator=gen, device="cuda")
    x = torch.empty(n, d, device="cuda")
    for s in range(0, n, 1 << 18):
        w = which[s:s + (1 << 18)]
        latent = torch.randn(len(w), 4, generator=gen, device="cuda")
        x[s:s + len(w)] = (centres[w] + torch.einsum("nl,nld->nd", latent, basis[w])
                           + 0.05 * torch.randn(len(w), d, generator=gen, device="cuda"))
    return x


def timed(fn, repeats):
    """(last result, {median, min, max} in ms over `repeats` calls) by HIP events on the current stream; one warm-up."""
    import torch

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
                 "repeats": repeats}


def child(name, repeats):
    import torch

    from muygpys_amd.neighbors import NN_Wrapper

    n, m, d, k, data, _ = SHAPES[name]
    gen = torch.Generator(device="cuda").manual_seed(20260 + len(name))
    X = make_table(n, d, data, gen)
    bi = torch.randperm(n, generator=gen, device="cuda")[:m].sort().values
    rows = torch.randperm(m, generator=gen, device="cuda")[:RECALL_QUERIES]
    rec = {"shape": name, "table_rows": n, "queries": m, "feature_count": d, "nn_count": k, "data": data,
           "device": torch.cuda.get_device_name(0)}

    exact = NN_Wrapper(X, k)
    (want, _), rec["exact"] = timed(lambda: exact.get_batch_nns(bi), repeats)
    rec["exact"]["overflow_queries"] = int(exact.last_overflow.sum()) if exact.last_overflow is not None else None
    want = want[rows].clone()
    del exact
    torch.cuda.empty_cache()

    builds = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        nn = NN_Wrapper(X, k, nn_method="ivf", nlist=None, nprobe=1)
        torch.cuda.synchronize()
        builds.append(1e3 * (time.perf_counter() - t0))
    rec["ivf_build"] = {"median_ms": round(statistics.median(builds), 3), "min_ms": round(min(builds), 3),
                        "max_ms": round(max(builds), 3), "repeats": repeats, "first_build_included": True}
    rec["nlist"] = nn.nlist
    sizes = (nn.cell_start[1:] - nn.cell_start[:-1]).double()
    rec["cell_rows"] = {"mean": float(sizes.mean()), "max": int(sizes.max()), "empty": int((sizes == 0).sum())}
    rec["ivf"] = []
    for nprobe in NPROBES:
        if nprobe > nn.nlist:
            continue
        nn.nprobe = nprobe
        (got, _), t = timed(lambda: nn.get_batch_nns(bi), repeats)
        hits = (got[rows][:, :, None] == want[:, None, :]).any(2).double().mean()
        t.update(nprobe=nprobe, recall_at_k=round(float(hits), 5), recall_queries=RECALL_QUERIES,
                 short_queries=int(nn.last_short.sum()), share_of_table_scanned=round(nprobe / nn.nlist, 5),
                 speedup_over_exact=round(rec["exact"]["median_ms"] / t["median_ms"], 3))
        rec["ivf"].append(t)
        print(json.dumps({"shape": name, **t}), flush=True)
    print("RESULT " + json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="*", default=list(SHAPES), choices=list(SHAPES))
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "knn_ivf_bench.json"))
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
            print(f"[ivfbench] {name}: exit status {p.returncode}; nothing further is started", file=sys.stderr)
            break
        results += [json.loads(ln[7:]) for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"tool": "tools/ivfbench.py", "nprobes": NPROBES, "shapes": results}, f, indent=1)
        f.write("\n")
    return 0 if len(results) == len(args.shapes) else 1


if __name__ == "__main__":
    sys.exit(main())
