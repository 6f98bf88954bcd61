#!/usr/bin/env python3
"""Timing of NN_Wrapper for nn_count > 64: the wide MFMA scan against the dense path (GPU box only).

    python tools/knnwidebench.py [--n 1000000] [--queries 1000000] [--d 8 40] [--k 65 100 128 256 512 1023]
                                 [--out profiles/knn_wide_bench.json]

Per (d, k), one table of --n Gaussian rows and --queries test queries (get_nns):

    wide    the route NN_Wrapper takes (mgp_knn_scan_wide + mgp_knn_finish_wide behind 4 096 head rows), all queries
            in one call.  Where a first pass over --probe queries predicts more than --wide-budget seconds for all of
            them, a slice of --wide-slice queries is timed instead and scaled (the entry says so).
    dense   the route before the wide scan existed, MUYGPYS_HIP_KNN_WIDE=0: (chunk x n) distances through rocBLAS, topk
            over n columns, a gather -- on a slice of --dense-passes chunks of the dense path's own chunk size (357 rows
            at n = 1 M), scaled to all queries: every pass is the same work, so the scaling is exact up to the last,
            partial pass.

The two legs alternate (dense, wide, dense, wide), every figure is a host clock around work that ends in a device
synchronise, after a warm-up of the same shape; both repeats are kept.  On the slice the dense leg answers, the two
routes' distances are compared (the largest relative difference is in the entry).

The sanity line: k = 64, where nothing is routed to the wide pair -- the narrow scans (scan_kind "bf16x3", the default,
and "f32", the wide kernel's arithmetic) beside the wide pair forced through `_scan_nns(force_wide=True)`.

An existing --out file is updated entry by entry, so the shapes can be measured over several runs."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from muygpys_amd.neighbors import NN_Wrapper


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def with_env(value, fn):
    old = os.environ.get("MUYGPYS_HIP_KNN_WIDE")
    os.environ["MUYGPYS_HIP_KNN_WIDE"] = value
    try:
        return fn()
    finally:
        if old is None:
            del os.environ["MUYGPYS_HIP_KNN_WIDE"]
        else:
            os.environ["MUYGPYS_HIP_KNN_WIDE"] = old


def bench_shape(X, Q, k, args):
    n, d = X.shape
    nn = NN_Wrapper(X, k)
    per_row = 3 * n * 4
    chunk = max(1, min(nn.chunk, nn.DENSE_BUDGET_BYTES // per_row))
    dense_q = min(Q.shape[0], chunk * args.dense_passes)
    probe = min(Q.shape[0], args.probe)

    def wide(rows):
        out = with_env("1", lambda: nn.get_nns(Q[:rows]))
        assert nn.last_route == "wide", nn.last_route
        return out

    def dense(rows):
        out = with_env("0", lambda: nn.get_nns(Q[:rows]))
        assert nn.last_route == "dense", nn.last_route
        return out

    dense(chunk)                      # warm-up: rocBLAS picks its kernel, topk its workspace
    t_probe = min(timed(lambda: wide(probe))[0], timed(lambda: wide(probe))[0])
    wide_q = Q.shape[0]
    if t_probe * Q.shape[0] / probe > args.wide_budget:
        wide_q = min(Q.shape[0], args.wide_slice)
    if wide_q > probe:
        wide(wide_q)                  # warm-up of the timed shape (allocator)
    t_dense, t_wide = [], []
    for _ in range(2):
        td, (di, dd) = timed(lambda: dense(dense_q))
        tw, (wi, wd) = timed(lambda: wide(wide_q))
        t_dense.append(td)
        t_wide.append(tw)
    m = min(dense_q, wide_q)
    rel = float(((wd[:m].double() - dd[:m].double()).abs() / dd[:m].double().clamp(min=1e-30)).max())
    same = float((wi[:m] == di[:m]).double().mean())
    scale_d, scale_w = Q.shape[0] / dense_q, Q.shape[0] / wide_q
    entry = {
        "n": n, "queries": Q.shape[0], "d": d, "k": k,
        "wide_ms": [round(1e3 * t * scale_w, 1) for t in t_wide], "wide_queries_timed": wide_q,
        "wide_scaled_from_slice": wide_q != Q.shape[0],
        "dense_ms": [round(1e3 * t * scale_d, 1) for t in t_dense], "dense_queries_timed": dense_q,
        "dense_scaled_from_slice": dense_q != Q.shape[0], "dense_chunk_rows": chunk,
        "speedup": round(min(t_dense) * scale_d / (min(t_wide) * scale_w), 2),
        "largest_relative_distance_difference": rel, "share_of_ranks_with_the_same_row": round(same, 5),
        "flagged": int(nn.last_overflow.sum()) if nn.last_overflow is not None else 0,
    }
    del nn
    return entry


def bench_sanity(X, Q, args):
    """k = 64: the narrow scans as routed, and the wide pair forced."""
    out = {"n": X.shape[0], "queries": Q.shape[0], "d": X.shape[1], "k": 64}
    for kind in ("bf16x3", "f32"):
        nn = NN_Wrapper(X, 64, scan_kind=kind)
        nn.get_nns(Q[:args.probe])
        assert nn.last_route == "scan"
        out[f"scan_{kind}_ms"] = [round(1e3 * timed(lambda: nn.get_nns(Q))[0], 1) for _ in range(2)]
    nn = NN_Wrapper(X, 64)
    qc = (Q - nn._mean).contiguous()
    nn._scan_nns(qc[:args.probe], 64, None, force_wide=True)
    assert nn.last_route == "wide"
    out["wide_forced_ms"] = [round(1e3 * timed(lambda: nn._scan_nns(qc, 64, None, force_wide=True))[0], 1) for _ in range(2)]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--queries", type=int, default=1_000_000)
    ap.add_argument("--d", type=int, nargs="+", default=[8, 40])
    ap.add_argument("--k", type=int, nargs="+", default=[65, 100, 128, 256, 512, 1023])
    ap.add_argument("--dense-passes", type=int, default=4)
    ap.add_argument("--probe", type=int, default=65536)
    ap.add_argument("--wide-budget", type=float, default=20.0, help="seconds one full wide call may take")
    ap.add_argument("--wide-slice", type=int, default=262144)
    ap.add_argument("--no-sanity", action="store_true")
    ap.add_argument("--out", default=os.path.join("profiles", "knn_wide_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this is a measurement: it needs the GPU"
    result = {"entries": {}, "sanity_k64": {}}
    if os.path.exists(args.out):
        with open(args.out) as f:
            result = json.load(f)
    result["device"] = torch.cuda.get_device_name(0)
    result["what"] = ("NN_Wrapper.get_nns, Gaussian table and queries; ms for all queries (scaled where an entry says "
                      "so), two repeats each, dense and wide alternating; speedup = best dense over best wide")

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1, sort_keys=True)

    for d in args.d:
        g = torch.Generator(device="cuda").manual_seed(d)
        X = torch.randn(args.n, d, device="cuda", generator=g)
        Q = torch.randn(args.queries, d, device="cuda", generator=g)
        if not args.no_sanity:
            result["sanity_k64"][f"d{d}"] = bench_sanity(X, Q, args)
            print(json.dumps(result["sanity_k64"][f"d{d}"]), flush=True)
            save()
        for k in args.k:
            entry = bench_shape(X, Q, k, args)
            result["entries"][f"d{d}_k{k}"] = entry
            print(json.dumps(entry), flush=True)
            save()
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
