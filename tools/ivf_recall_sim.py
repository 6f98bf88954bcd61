#!/usr/bin/env python3
"""How much of the table must an inverted-cell (IVF) search scan for a given recall?  A CPU-only torch simulation of the
search nn_method="ivf" runs on the GPU (muygpys_amd/neighbors.py): k-means cells (Lloyd passes from random rows), every
query scans the rows of its `nprobe` nearest cells, exact neighbours within them.  Queries are table rows, the row
itself excluded; recall is against the exact neighbours.  Each line: recall / share of the table scanned.

Also the exact variant nobody should rebuild: cells visited in order of |q - c| - radius until the bound passes the
running k-th distance (what an exact search pruned by bounds would have to visit).

    python tools/ivf_recall_sim.py [--n 200000] [--queries 1000] [--out profiles/knn_ivf_recall_sim.txt]
"""
import argparse
import os
import sys
import time

import torch


def gaussian(n, d, gen):
    return torch.randn(n, d, generator=gen)


def uniform(n, d, gen):
    return torch.rand(n, d, generator=gen)


def mixture(n, d, gen, clusters=30):
    """Clusters with a few principal directions each: low intrinsic dimension at any d."""
    centres = 4.0 * torch.randn(clusters, d, generator=gen)
    which = torch.randint(0, clusters, (n,), generator=gen)
    basis = torch.randn(clusters, 4, d, generator=gen) / 2.0
    latent = torch.randn(n, 4, generator=gen)
    return centres[which] + torch.einsum("nl,nld->nd", latent, basis[which]) + 0.05 * torch.randn(n, d, generator=gen)


def nearest(x, c, chunk=16384):
    csq = (c * c).sum(1)
    return torch.cat([(csq[None, :] - 2.0 * x[s:s + chunk] @ c.T).argmin(1) for s in range(0, len(x), chunk)])


def kmeans(x, nlist, iters, gen):
    c = x[torch.randperm(len(x), generator=gen)[:nlist]].clone()
    for _ in range(iters):
        cell = nearest(x, c)
        sums = torch.zeros_like(c).index_add_(0, cell, x)
        count = torch.bincount(cell, minlength=nlist)
        c = torch.where(count[:, None] > 0, sums / count.clamp(min=1)[:, None], c)
    return c, nearest(x, c)


def simulate(x, k, nlist, nprobes, queries, gen, iters=10, pruned=False):
    n = len(x)
    c, cell = kmeans(x, nlist, iters, gen)
    order = cell.argsort(stable=True)
    start = torch.zeros(nlist + 1, dtype=torch.int64)
    start[1:] = torch.bincount(cell, minlength=nlist).cumsum(0)
    qi = torch.randperm(n, generator=gen)[:queries]
    q = x[qi]
    d2 = torch.cdist(q.double(), x.double()) ** 2
    d2[torch.arange(queries), qi] = float("inf")
    exact_d, exact_i = d2.topk(k, dim=1, largest=False)
    cd = torch.cdist(q.double(), c.double())
    ranked = (cd ** 2).argsort(1)
    out = {}
    for nprobe in nprobes:
        hit = scanned = 0
        for r in range(queries):
            rows = torch.cat([order[start[j]:start[j + 1]] for j in ranked[r, :nprobe]])
            scanned += len(rows)
            dd = d2[r, rows]
            found = rows[dd.topk(min(k, len(rows)), largest=False).indices]
            hit += len(set(found.tolist()) & set(exact_i[r].tolist()))
        out[nprobe] = (hit / (queries * k), scanned / (queries * n))
    visited = None
    if pruned:
        radius = torch.zeros(nlist, dtype=torch.float64)
        dist_to_own = (x.double() - c.double()[cell]).norm(dim=1)
        radius.scatter_reduce_(0, cell, dist_to_own, reduce="amax")
        bound = (cd - radius[None, :]).clamp(min=0)
        visited = 0
        for r in range(queries):
            kth = exact_d[r, -1].sqrt()
            # cells in order of the bound; the visit stops once the bound passes the running k-th distance, which is
            # never below the final one: every cell with bound <= the final k-th distance is visited at the least
            visited += int((start[1:] - start[:-1])[bound[r] <= kth].sum())
        visited /= queries * n
    return out, visited


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=200_000)
    ap.add_argument("--queries", type=int, default=1000)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "knn_ivf_recall_sim.txt"))
    args = ap.parse_args()
    torch.set_num_threads(min(16, torch.get_num_threads()))
    n, m = args.n, args.queries
    lines = [f"# tools/ivf_recall_sim.py --n {n} --queries {m} --iters {args.iters}  (CPU, torch {torch.__version__})",
             "# recall@k against exact neighbours / share of table rows scanned; queries are table rows, self excluded",
             ""]

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit("## approximate probing")
    cases = [("Gaussian", gaussian, 8, 50, 448, (8, 16, 32)), ("Gaussian", gaussian, 8, 50, 1024, (8, 16, 32)),
             ("30-cluster mixture", mixture, 8, 50, 448, (8, 16, 32)), ("Gaussian", gaussian, 4, 30, 448, (8, 16)),
             ("30-cluster mixture", mixture, 40, 30, 448, (8, 16, 32)), ("Gaussian", gaussian, 40, 30, 64, (8, 16, 32)),
             ("Gaussian", gaussian, 40, 30, 448, (8, 16, 32))]
    for name, make, d, k, nlist, nprobes in cases:
        gen = torch.Generator().manual_seed(1000 * d + nlist)
        t0 = time.time()
        res, _ = simulate(make(n, d, gen), k, nlist, nprobes, m, gen, args.iters)
        cells = "  ".join(f"nprobe {p}: {r:.4f} / {100 * s:.2f} %" for p, (r, s) in res.items())
        emit(f"{name:>20s} d = {d:2d} k = {k:2d} nlist = {nlist:4d}   {cells}   ({time.time() - t0:.0f} s)")
    emit("")
    emit("## exact search pruned by bounds (cells of 1 024; share of table rows that must be visited)")
    for name, make, d, k in (("Gaussian", gaussian, 8, 50), ("uniform", uniform, 8, 50), ("Gaussian", gaussian, 16, 50),
                             ("Gaussian", gaussian, 4, 50)):
        gen = torch.Generator().manual_seed(77 + d)
        _, visited = simulate(make(n, d, gen), k, 1024, (), m, gen, args.iters, pruned=True)
        emit(f"{name:>20s} d = {d:2d} k = {k:2d}   {100 * visited:.1f} %")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    sys.exit(main())
