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

``--cell-scan block`` measures the block cell scan (``NN_Wrapper.cell_scan = "block"``) instead: per shape and nprobe
the per-query scan, the block scan and the exact scan alternate in one process for ``--repeats`` rounds after a warm-up
round, HIP events around the whole call; medians, the block / per-query ratio with the per-query side's
(max - min) / median next to it, recall of both, the entries in which their results differ, the share of queries the
block launch flagged in ``last_overflow`` and the mean size of a block's cell union relative to nprobe.  Writes
profiles/knn_ivf_block_bench.json.

``--cell-scan wide --nn-count K [K ...]`` measures the wide cell scan (``cell_scan="wide"``, 1 <= K <= 1024) against the
exact wide scan (``last_route == "wide"``) of the same table: per shape, K and nprobe the two alternate in one process
for ``--repeats`` rounds after a warm-up round; medians, the exact / index ratio with the exact side's
(max - min) / median next to it, recall@K on 4 000 sampled queries, the index build time.  Writes
profiles/knn_ivf_wide_bench.json.

``--cell-scan long --nn-count K [K ...]`` measures the long-row cell scan (``cell_scan="long"``, 65 <= d <= 256) the same
way against the exact long-row scan (``last_route == "long"``) on the d = 100 and d = 256 shapes ->
profiles/knn_ivf_long_bench.json.  ``MUYGPYS_HIP_LIB`` selects an A/B build of the library (tools/mkvariant.sh), as for
every tool: the scan without its prune test is measured by the same command under ``--out``.
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
# --cell-scan long (nn_count comes from --nn-count)
LONG_SHAPES = {
    "d100_mixture": (1_000_000, 1_000_000, 100, 30, "mixture", 540),
    "d100_gaussian": (1_000_000, 1_000_000, 100, 30, "gaussian", 540),
    "d256_mixture": (1_000_000, 1_000_000, 256, 30, "mixture", 900),
    "d256_gaussian": (1_000_000, 1_000_000, 256, 30, "gaussian", 900),
}
SHAPES.update(LONG_SHAPES)


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


def event_ms(fn):
    import torch

    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return out, a.elapsed_time(b)


def union_per_probe(nn, bi, blocks=512):
    """Mean number of distinct cells a block of 128 queries (in the search's order: by nearest cell) walks, its seed
    cells aside, relative to nprobe -- on `blocks` blocks spread evenly over the batch."""
    import torch

    q = nn.train[nn._inv[bi]]
    probes, nearest = nn._probe(q)
    order = nearest.argsort()
    ps, seed = probes[order].to(torch.int64), nearest[order]
    nblocks = ps.shape[0] // 128
    pick = torch.arange(0, nblocks, max(1, nblocks // blocks), device=ps.device)
    rows = (pick[:, None] * 128 + torch.arange(128, device=ps.device)[None, :]).reshape(-1)
    keys = (rows // 128)[:, None] * nn.nlist + ps[rows]
    keys = keys[ps[rows] != seed[rows][:, None]]
    return float(torch.unique(keys).numel()) / float(pick.numel()) / nn.nprobe


def child_block(name, rounds):
    """The per-query cell scan, the block cell scan and the exact scan, alternating in one process: per nprobe the
    medians over `rounds` rounds (one warm-up round first), block / query ratios next to the per-query side's spread."""
    import torch

    from muygpys_amd.neighbors import NN_Wrapper

    n, m, d, k, data, _ = SHAPES[name]
    gen = torch.Generator(device="cuda").manual_seed(20260 + len(name))
    X = make_table(n, d, data, gen)
    bi = torch.randperm(n, generator=gen, device="cuda")[:m].sort().values
    rows = torch.randperm(m, generator=gen, device="cuda")[:RECALL_QUERIES]
    rec = {"shape": name, "table_rows": n, "queries": m, "feature_count": d, "nn_count": k, "data": data,
           "device": torch.cuda.get_device_name(0), "rounds": rounds}
    exact = NN_Wrapper(X, k)
    want = exact.get_batch_nns(bi)[0][rows].clone()
    nn = NN_Wrapper(X, k, nn_method="ivf", nlist=None, nprobe=1)
    rec["nlist"] = nn.nlist

    def recall(got):
        return round(float((got[rows][:, :, None] == want[:, None, :]).any(2).double().mean()), 5)

    def stats(ms):
        return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3)}

    rec["ivf"] = []
    for nprobe in NPROBES:
        if nprobe > nn.nlist:
            continue
        nn.nprobe = nprobe
        ms = {"query": [], "block": [], "exact": []}
        got, over = {}, 0
        for rnd in range(rounds + 1):  # (round 0 warms up)
            for side in ("query", "block", "exact"):
                if side == "exact":
                    _, t = event_ms(lambda: exact.get_batch_nns(bi))
                else:
                    nn.cell_scan = side
                    (got[side], _), t = event_ms(lambda: nn.get_batch_nns(bi))
                    if side == "block":
                        over = int(nn.last_overflow.sum())
                if rnd:
                    ms[side].append(t)
        qs, bs, es = stats(ms["query"]), stats(ms["block"]), stats(ms["exact"])
        row = {"nprobe": nprobe, "query": qs, "block": bs, "exact": es,
               "block_over_query_speedup": round(qs["median_ms"] / bs["median_ms"], 3),
               "query_spread": round((qs["max_ms"] - qs["min_ms"]) / qs["median_ms"], 4),
               "block_over_exact_speedup": round(es["median_ms"] / bs["median_ms"], 3),
               "query_over_exact_speedup": round(es["median_ms"] / qs["median_ms"], 3),
               "recall_at_k": {"query": recall(got["query"]), "block": recall(got["block"])},
               "entries_that_differ": int((got["query"] != got["block"]).sum()), "entries": int(got["query"].numel()),
               "overflow_share": round(over / m, 5), "short_queries": int(nn.last_short.sum()),
               "union_cells_per_probe": round(union_per_probe(nn, bi), 3)}
        rec["ivf"].append(row)
        print(json.dumps({"shape": name, **row}), flush=True)
    print("RESULT " + json.dumps(rec), flush=True)


def child_wide(name, rounds, k, scan="wide"):
    """The wide cell scan (cell_scan="wide") at nn_count = k and the exact wide scan -- or (`scan` = "long") the long-row
    cell scan and the exact long-row scan -- alternating in one process: per nprobe the medians over `rounds` rounds
    (one warm-up round first), exact / index ratio next to the exact side's spread, recall against the exact result."""
    import torch

    from muygpys_amd.neighbors import NN_Wrapper

    n, m, d, _, data, _ = SHAPES[name]
    gen = torch.Generator(device="cuda").manual_seed(20260 + len(name))
    X = make_table(n, d, data, gen)
    bi = torch.randperm(n, generator=gen, device="cuda")[:m].sort().values
    rows = torch.randperm(m, generator=gen, device="cuda")[:RECALL_QUERIES]
    rec = {"shape": name, "table_rows": n, "queries": m, "feature_count": d, "nn_count": k, "data": data,
           "device": torch.cuda.get_device_name(0), "rounds": rounds}
    exact = NN_Wrapper(X, k)
    want = exact.get_batch_nns(bi)[0][rows].clone()
    rec["exact_route"] = exact.last_route
    if (scan == "long" or k > 64) and exact.last_route != scan:
        raise RuntimeError(f"the yardstick is the exact {scan} scan, got last_route = {exact.last_route!r}")
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    nn = NN_Wrapper(X, k, nn_method="ivf", nlist=None, nprobe=1, cell_scan=scan)
    torch.cuda.synchronize()
    rec["ivf_build_ms"] = round(1e3 * (time.perf_counter() - t0), 3)
    rec["nlist"] = nn.nlist

    def stats(ms):
        return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3)}

    rec["ivf"] = []
    for nprobe in NPROBES:
        if nprobe > nn.nlist:
            continue
        nn.nprobe = nprobe
        ms = {scan: [], "exact": []}
        for rnd in range(rounds + 1):  # (round 0 warms up)
            (got, _), t = event_ms(lambda: nn.get_batch_nns(bi))
            got = got[rows].clone()
            _, te = event_ms(lambda: exact.get_batch_nns(bi))
            if rnd:
                ms[scan].append(t)
                ms["exact"].append(te)
        ws, es = stats(ms[scan]), stats(ms["exact"])
        row = {"nprobe": nprobe, scan: ws, "exact": es,
               f"{scan}_over_exact_speedup": round(es["median_ms"] / ws["median_ms"], 3),
               "exact_spread": round((es["max_ms"] - es["min_ms"]) / es["median_ms"], 4),
               # (in slices of 256 queries: the (queries, k, k) comparison is 4 GB at k = 1023)
               "recall_at_k": round(sum(float((got[s:s + 256, :, None] == want[s:s + 256, None, :]).any(2).sum())
                                        for s in range(0, len(got), 256)) / got.numel(), 5),
               "short_queries": int(nn.last_short.sum()), "share_of_table_scanned": round(nprobe / nn.nlist, 5)}
        rec["ivf"].append(row)
        print(json.dumps({"shape": name, "nn_count": k, **row}), flush=True)
    print("RESULT " + json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="*", default=None, choices=list(SHAPES),
                    help="default: the d = 100 and d = 256 shapes under --cell-scan long, every other shape otherwise")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--cell-scan", default="query", choices=["query", "block", "wide", "long"],
                    help="block: the block cell scan against the per-query one and the exact scan, alternating "
                         "(--repeats rounds) -> profiles/knn_ivf_block_bench.json; wide: the wide cell scan at "
                         "--nn-count against the exact wide scan, alternating -> profiles/knn_ivf_wide_bench.json; long: "
                         "the long-row cell scan against the exact long-row scan -> profiles/knn_ivf_long_bench.json")
    ap.add_argument("--nn-count", type=int, nargs="+", default=[100], help="--cell-scan wide | long: the list lengths (1 .. 1024)")
    ap.add_argument("--out", default="")
    ap.add_argument("--child", default="", help=argparse.SUPPRESS)
    args = ap.parse_args()
    lists = args.cell_scan in ("wide", "long")  # (one child per shape and list length)
    if args.shapes is None:
        args.shapes = [name for name in SHAPES if (name in LONG_SHAPES) == (args.cell_scan == "long")]
    if args.child and lists:
        return child_wide(args.child, args.repeats, args.nn_count[0], args.cell_scan)
    if args.child:
        return (child_block if args.cell_scan == "block" else child)(args.child, args.repeats)
    if not args.out:
        args.out = os.path.join(ROOT, "profiles", {"block": "knn_ivf_block_bench.json", "wide": "knn_ivf_wide_bench.json",
                                                      "long": "knn_ivf_long_bench.json"}
                                .get(args.cell_scan, "knn_ivf_bench.json"))
    results = []
    runs = [(name, k) for name in args.shapes for k in (args.nn_count if lists else [None])]
    for name, k in runs:  # chained: a child that fails, faults or runs out of time ends the run
        cmd = ["timeout", "-k", "10", str(SHAPES[name][5]), sys.executable, os.path.abspath(__file__), "--child", name,
               "--repeats", str(args.repeats), "--cell-scan", args.cell_scan]
        p = subprocess.run(cmd + ([] if k is None else ["--nn-count", str(k)]), stdout=subprocess.PIPE, text=True)
        sys.stdout.write(p.stdout)
        sys.stdout.flush()
        if p.returncode != 0:
            print(f"[ivfbench] {name}: exit status {p.returncode}; nothing further is started", file=sys.stderr)
            break
        results += [json.loads(ln[7:]) for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        tool = "tools/ivfbench.py" + (f" --cell-scan {args.cell_scan}" if args.cell_scan != "query" else "")
        json.dump({"tool": tool, "library": os.environ.get("MUYGPYS_HIP_LIB", "") or "the regular build",
                   "nprobes": NPROBES, "shapes": results}, f, indent=1)
        f.write("\n")
    return 0 if len(results) == len(runs) else 1


if __name__ == "__main__":
    sys.exit(main())
