#!/usr/bin/env python3
"""Timing of NN_Wrapper on the feature counts the exact scans took up last: padded rows (d % 4 != 0, d < 4) and long
rows (64 < d <= 256), against the dense path (GPU box only).

    python tools/knnlongbench.py [--n 1000000] [--queries 1000000] [--d 2 3 10 30 68 100 128 192 256] [--k 30 100]
                                 [--out profiles/knn_long_bench.json]

One process per (d, k) line, each under its own time limit (--line-timeout); the driver stops at the first line that
does not end cleanly.  Per line, one table of --n Gaussian rows and --queries test queries (get_nns):

    new     the route NN_Wrapper takes by default ("scan" / "wide" on rows zero-padded to a multiple of four, "long"
            beyond 64 features: mgp_knn_scan_long / mgp_knn_scan_long_wide behind 4 096 head rows), all queries in
            one call: a warm-up on --probe queries, then --repeats calls, the median reported.
    dense   NN_Wrapper(use_scan=False) on the same build -- what these shapes ran before they were routed: (chunk x n)
            distances through rocBLAS, topk over n columns, a gather -- on a slice of --dense-passes chunks of the dense
            path's own chunk size (357 rows at n = 1 M), scaled to all queries (every pass is the same work, so the
            scaling is exact up to the last, partial pass; the entry says so), after a warm-up pass; the median of
            --repeats.

Every figure is a host clock around work that ends in a device synchronise.  On the slice the dense leg answers, the two
routes' distances are compared (the largest relative difference is in the entry).

An existing --out file is updated entry by entry, so the shapes can be measured over several runs."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn):
    import torch

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def bench_line(d, k, args):
    import torch

    from muygpys_amd.neighbors import NN_Wrapper, scan_route

    g = torch.Generator(device="cuda").manual_seed(d)
    X = torch.randn(args.n, d, device="cuda", generator=g)
    Q = torch.randn(args.queries, d, device="cuda", generator=g)
    want = scan_route(d, k, torch.float32, args.n, True)
    new, old = NN_Wrapper(X, k), NN_Wrapper(X, k, use_scan=False)
    chunk = max(1, min(old.chunk, old.DENSE_BUDGET_BYTES // (3 * args.n * 4)))
    dense_q = min(Q.shape[0], chunk * args.dense_passes)
    old.get_nns(Q[:chunk])  # warm-up: rocBLAS picks its kernel, topk its workspace
    assert old.last_route == "dense", old.last_route
    new.get_nns(Q[:min(Q.shape[0], args.probe)])
    assert new.last_route == want, (new.last_route, want)
    t_new, t_dense = [], []
    for _ in range(args.repeats):
        td, (di, dd) = timed(lambda: old.get_nns(Q[:dense_q]))
        tn, (ni, nd) = timed(lambda: new.get_nns(Q))
        t_dense.append(td)
        t_new.append(tn)
    rel = float(((nd[:dense_q].double() - dd.double()).abs() / dd.double().clamp(min=1e-30)).max())
    same = float((ni[:dense_q] == di).double().mean())
    scale = Q.shape[0] / dense_q
    new_ms, dense_ms = 1e3 * statistics.median(t_new), 1e3 * statistics.median(t_dense) * scale
    return {
        "n": args.n, "queries": Q.shape[0], "d": d, "stored_width": new.train.shape[1], "k": k, "route": str(want),
        "new_ms": round(new_ms, 1), "new_ms_repeats": [round(1e3 * t, 1) for t in t_new],
        "dense_ms": round(dense_ms, 1), "dense_ms_repeats": [round(1e3 * t * scale, 1) for t in t_dense],
        "dense_queries_timed": dense_q, "dense_scaled_from_slice": dense_q != Q.shape[0], "dense_chunk_rows": chunk,
        "speedup": round(dense_ms / new_ms, 2),
        "largest_relative_distance_difference": rel, "share_of_ranks_with_the_same_row": round(same, 5),
        "flagged": int(new.last_overflow.sum()) if new.last_overflow is not None else 0,
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--queries", type=int, default=1_000_000)
    ap.add_argument("--d", type=int, nargs="+", default=[2, 3, 10, 30, 68, 100, 128, 192, 256])
    ap.add_argument("--k", type=int, nargs="+", default=[30, 100])
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--dense-passes", type=int, default=4)
    ap.add_argument("--probe", type=int, default=65536)
    ap.add_argument("--line-timeout", type=float, default=240.0, help="seconds one (d, k) process may take")
    ap.add_argument("--line", type=int, nargs=2, metavar=("D", "K"), help="measure this one line and print it (the child)")
    ap.add_argument("--out", default=os.path.join("profiles", "knn_long_bench.json"))
    args = ap.parse_args()
    if args.line:
        import torch

        assert torch.cuda.is_available(), "this is a measurement: it needs the GPU"
        entry = bench_line(args.line[0], args.line[1], args)
        entry["device"] = torch.cuda.get_device_name(0)
        print("LINE " + json.dumps(entry), flush=True)
        return 0
    result = {"entries": {}}
    if os.path.exists(args.out):
        with open(args.out) as f:
            result = json.load(f)
    result["what"] = ("NN_Wrapper.get_nns, Gaussian table and queries, fp32; ms for all queries, the median of the repeats; "
                      "new = the default route on all queries, dense = use_scan=False on a slice of whole passes, scaled "
                      "(dense_scaled_from_slice); one process per line; speedup = dense over new")
    for d in args.d:
        for k in args.k:
            cmd = [sys.executable, os.path.abspath(__file__), "--line", str(d), str(k), "--n", str(args.n), "--queries",
                   str(args.queries), "--repeats", str(args.repeats), "--dense-passes", str(args.dense_passes), "--probe",
                   str(args.probe)]
            try:
                p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=args.line_timeout)
            except subprocess.TimeoutExpired:
                print(f"d = {d}, k = {k}: no result within {args.line_timeout:.0f} s; stopping", flush=True)
                return 1
            lines = [ln for ln in p.stdout.splitlines() if ln.startswith("LINE ")]
            if p.returncode != 0 or not lines:
                print(f"d = {d}, k = {k}: exit status {p.returncode}; stopping\n{p.stdout[-2000:]}", flush=True)
                return 1
            entry = json.loads(lines[-1][5:])
            result["device"] = entry.pop("device")
            result["entries"][f"d{d}_k{k}"] = entry
            print(json.dumps(entry), flush=True)
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                json.dump(result, f, indent=1, sort_keys=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
