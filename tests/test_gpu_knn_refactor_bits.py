"""GPU: every k-NN entry of the C ABI returns the bits it returned before the kernels were moved onto their shared
headers (csrc/mgp_knn_common.h, mgp_knn_tile.h, mgp_knn_cells_scan.h).

tests/golden/parent_bits/knn_bits.npz was recorded by `record()` below on the commit before that change, on an MI355X.
Every case here is a launch or two on a table of a thousand rows; its inputs come from seeded CPU generators (the seed
is crc32 of the case's name), its initial lists from fp64 distances on the CPU, so nothing but the entry under test
shapes the result.  The comparison is exact: row numbers, and distances as their int32 bit patterns, slot by slot (the
lists are unordered, so this also pins which lane or slot an entry lands in), plus the overflow / short flags and shell
counts where an entry has them.

    scan_f32     n = 1000 (15 tiles and 40 rows), m = 130 (one workgroup and two queries), d = 4, 40, k = 1, 30, 64,
                 with and without self_idx, lists started from the first 512 rows
    scan_wide    the same tables, d = 40, k = 65, 200, lists started from the first 256 rows
    scan_long    mgp_knn_scan_long (k = 30) and mgp_knn_scan_long_wide (k = 30, 100) at d = 68, 100
    cells        ten cells of 100, 0, 250, 64, 65, 1, 129, 200, 63, 128 rows (an empty one, two that merge mid-cell), five
                 queries (a partly filled workgroup, two of them rows of the table), nprobe = 1, 3 with an out-of-range
                 probe in one row, d = 8 (query row in registers), 40 (in LDS), k = 1, 10, 64
    cells_wide   the same index at k = 64, 65, 200; k = 1024 on 1500 rows (cell 2 holds 750): some queries are short,
                 the others select at the end
    cells_block  the same index, 40 queries seeded by mgp_knn_cells_scan on one of their cells (for query 0 the cell of
                 one row), k = 10
    grid         a 4 x 4 grid over 1000 points of the unit square, 20 queries, k = 10
    wrapper      NN_Wrapper.get_nns on the exact route (9000 x 8 table) at k = 30 and k = 100: the finish step"""

import functools
import os
import zlib

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "parent_bits", "knn_bits.npz")
CELLS = [100, 0, 250, 64, 65, 1, 129, 200, 63, 128]
PROBES = {1: [[2], [1], [-3], [7], [4]], 3: [[2, 1, 7], [6, 3, 4], [0, 12, 9], [5, 8, 2], [7, 2, 0]]}


def gen(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()))


def bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.int32).copy()


def ints(t):
    return t.detach().cpu().numpy().astype(np.int32)


def scan_case(entry, d, k, own, start):
    """One call of an exact-scan entry on lists that hold the fp64 k-best of rows [0, start)."""
    from muygpys_amd import _lib

    name = f"{entry}/d{d}/k{k}/{'self' if own else 'test'}"
    g = gen(f"scan/d{d}/{'self' if own else 'test'}")  # (one table per (d, own): shared by the entries and every k)
    n, m = 1000, 130
    X = torch.randn(n, d, generator=g)
    rows = torch.randperm(n, generator=g)[:m]
    Q = X[rows].clone() if own else torch.randn(m, d, generator=g)
    d2 = ((Q[:, None, :].double() - X[None, :start].double()) ** 2).sum(-1)
    if own:
        inside = rows < start
        d2[torch.arange(m)[inside], rows[inside]] = float("inf")
    bd, bi = d2.topk(k, dim=1, largest=False)
    sq = torch.cat([(X.double() ** 2).sum(1).float(), torch.full(((-n) % 64,), float("inf"))]).cuda()
    qn = (Q.double() ** 2).sum(1).float().cuda()
    X, Q = X.cuda(), Q.cuda()
    best_d, best_i = bd.float().cuda().contiguous(), bi.to(torch.int32).cuda().contiguous()
    overflow = torch.zeros((m,), dtype=torch.int32, device="cuda")
    self_idx = rows.to(torch.int64).cuda() if own else None
    rc = getattr(_lib.load(), entry)(_lib.ptr(X), _lib.ptr(sq), n, d, _lib.ptr(Q), _lib.ptr(qn), _lib.ptr(self_idx), m, k,
                                     start, _lib.ptr(best_d), _lib.ptr(best_i), _lib.ptr(overflow), _lib.stream_ptr())
    assert rc == 0, (name, rc)
    torch.cuda.synchronize()
    return {f"{name}/best_d": bits(best_d), f"{name}/best_i": ints(best_i), f"{name}/overflow": ints(overflow)}


def scan_f32():
    out = {}
    for d in (4, 40):
        for k in (1, 30, 64):
            for own in (False, True):
                out.update(scan_case("mgp_knn_scan_f32", d, k, own, 512))
    return out


def scan_wide():
    out = {}
    for k in (65, 200):
        for own in (False, True):
            out.update(scan_case("mgp_knn_scan_wide", 40, k, own, 256))
    return out


def scan_long():
    out = {}
    for d in (68, 100):
        out.update(scan_case("mgp_knn_scan_long", d, 30, False, 256))
        for k in (30, 100):
            out.update(scan_case("mgp_knn_scan_long_wide", d, k, True, 256))
    return out


def cell_index(d, lengths=CELLS):
    """A table stored cell by cell, five queries (3 and 4 are rows of cells 2 and 7) and their stored positions."""
    g = gen(f"cells/d{d}/n{sum(lengths)}")
    X = torch.randn(sum(lengths), d, generator=g)
    start = torch.tensor(np.concatenate([[0], np.cumsum(lengths)]), dtype=torch.int64)
    Q = torch.randn(5, d, generator=g)
    self_pos = torch.tensor([-1, -1, -1, int(start[2]) + 70, int(start[7]) + 199], dtype=torch.int64)
    Q[3], Q[4] = X[self_pos[3]], X[self_pos[4]]
    return X, start, Q, self_pos


def cells_case(entry, d, k, nprobe, lengths=CELLS):
    from muygpys_amd import _lib

    name = f"{entry}/d{d}/k{k}/p{nprobe}/n{sum(lengths)}"
    X, start, Q, self_pos = (t.cuda() for t in cell_index(d, lengths))
    probes = torch.tensor(PROBES[nprobe], dtype=torch.int32, device="cuda")
    m = Q.shape[0]
    best_d = torch.full((m, k), -7.0, device="cuda")
    best_i = torch.full((m, k), -7, device="cuda", dtype=torch.int32)
    short = torch.full((m,), -7, device="cuda", dtype=torch.int32)
    rc = getattr(_lib.load(), entry)(_lib.ptr(X), X.shape[0], d, _lib.ptr(start), len(lengths), _lib.ptr(Q), m,
                                     _lib.ptr(probes), nprobe, _lib.ptr(self_pos), k, _lib.ptr(best_d), _lib.ptr(best_i),
                                     _lib.ptr(short), _lib.stream_ptr())
    assert rc == 0, (name, rc)
    torch.cuda.synchronize()
    return {f"{name}/best_d": bits(best_d), f"{name}/best_i": ints(best_i), f"{name}/short_flag": ints(short)}


def cells():
    out = {}
    for d in (8, 40):
        for nprobe in (1, 3):
            for k in (1, 10, 64):
                out.update(cells_case("mgp_knn_cells_scan", d, k, nprobe))
    return out


def cells_wide():
    out = {}
    big = [750 if c == 2 else n for c, n in enumerate(CELLS)]
    for d in (8, 40):
        for nprobe in (1, 3):
            for k in (64, 65, 200):
                out.update(cells_case("mgp_knn_cells_scan_wide", d, k, nprobe))
        got = cells_case("mgp_knn_cells_scan_wide", d, 1024, 3, big)
        flags = got[f"mgp_knn_cells_scan_wide/d{d}/k1024/p3/n1500/short_flag"]
        assert flags.any() and not flags.all()  # (950 candidates or fewer for some queries, 1050 and more for others)
        out.update(got)
    return out


def cells_block():
    """Seeded the way tests/test_gpu_knn_cells_block.py seeds: mgp_knn_cells_scan on one cell per query, then the block
    scan over the others."""
    from muygpys_amd import _lib

    lib, out, k, m = _lib.load(), {}, 10, 40
    for d in (8, 40):
        name = f"mgp_knn_cells_scan_block/d{d}/k{k}"
        X, start, _, _ = cell_index(d)
        g = gen(f"block/d{d}")
        Q = torch.randn(m, d, generator=g)
        probes = torch.rand(m, len(CELLS), generator=g).argsort(1)[:, :3].sort(1).values.to(torch.int32)
        probes[0] = torch.tensor([3, 5, 6], dtype=torch.int32)
        seed_cell = probes[:, 1].clone()  # (query 0: cell 5, one row -- its list starts short of k)
        sq = torch.cat([(X.double() ** 2).sum(1).float(), torch.full((1,), float("inf"))]).cuda()
        qn = (Q.double() ** 2).sum(1).float().cuda()
        X, start, Q, probes, n = X.cuda(), start.cuda(), Q.cuda(), probes.cuda().contiguous(), X.shape[0]
        best_d = torch.empty((m, k), device="cuda")
        best_i = torch.empty((m, k), device="cuda", dtype=torch.int32)
        flag = torch.empty((m,), device="cuda", dtype=torch.int32)
        seed = seed_cell[:, None].cuda().contiguous()
        rc = lib.mgp_knn_cells_scan(_lib.ptr(X), n, d, _lib.ptr(start), len(CELLS), _lib.ptr(Q), m, _lib.ptr(seed), 1, None,
                                    k, _lib.ptr(best_d), _lib.ptr(best_i), _lib.ptr(flag), _lib.stream_ptr())
        assert rc == 0, (name, rc)
        skip = seed_cell.to(torch.int64).cuda()
        overflow = torch.full((m,), -7, device="cuda", dtype=torch.int32)
        rc = lib.mgp_knn_cells_scan_block(_lib.ptr(X), _lib.ptr(sq), n, d, _lib.ptr(start), len(CELLS), _lib.ptr(Q),
                                          _lib.ptr(qn), m, _lib.ptr(probes), 3, _lib.ptr(skip), None, k, _lib.ptr(best_d),
                                          _lib.ptr(best_i), _lib.ptr(overflow), _lib.stream_ptr())
        assert rc == 0, (name, rc)
        torch.cuda.synchronize()
        assert int(flag[0]) == 1
        out.update({f"{name}/best_d": bits(best_d), f"{name}/best_i": ints(best_i), f"{name}/overflow": ints(overflow)})
    return out


def grid():
    from muygpys_amd import _lib

    g = gen("grid")
    n, m, k, dims = 1000, 20, 10, (4, 4, 1)
    edges = torch.tensor([0.25, 0.5, 0.75])
    P, Q = torch.rand(n, 2, generator=g), torch.rand(m, 2, generator=g)
    cell = lambda p: torch.stack([torch.bucketize(p[:, 0].contiguous(), edges, right=True),
                                  torch.bucketize(p[:, 1].contiguous(), edges, right=True),
                                  torch.zeros(len(p), dtype=torch.int64)], 1)
    linear = lambda c: (c[:, 2] * dims[1] + c[:, 1]) * dims[0] + c[:, 0]
    order = linear(cell(P)).argsort(stable=True)
    P = P[order]
    start = torch.cat([torch.zeros(1, dtype=torch.int64), torch.bincount(linear(cell(P)), minlength=16).cumsum(0)])
    pad = lambda p: torch.cat([p, torch.zeros(len(p), 2)], 1).cuda().contiguous()
    table, q, qcell = pad(P), pad(Q), cell(Q).to(torch.int32).cuda().contiguous()
    flat = torch.cat([edges, edges]).cuda()  # (g0 - 1 edges of axis 0, g1 - 1 of axis 1, none of axis 2)
    start = start.cuda()
    best_d = torch.full((m, k), -7.0, device="cuda")
    best_i = torch.full((m, k), -7, device="cuda", dtype=torch.int32)
    shells = torch.full((m,), -7, device="cuda", dtype=torch.int32)
    rc = _lib.load().mgp_knn_grid_scan(_lib.ptr(table), n, _lib.ptr(start), *dims, _lib.ptr(flat), _lib.ptr(q), m,
                                       _lib.ptr(qcell), None, k, _lib.ptr(best_d), _lib.ptr(best_i), _lib.ptr(shells),
                                       _lib.stream_ptr())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return {"mgp_knn_grid_scan/best_d": bits(best_d), "mgp_knn_grid_scan/best_i": ints(best_i),
            "mgp_knn_grid_scan/shells": ints(shells)}


def wrapper():
    from muygpys_amd.neighbors import NN_Wrapper

    g = gen("wrapper")
    X, Q = torch.randn(9000, 8, generator=g).cuda(), torch.randn(130, 8, generator=g).cuda()
    out = {}
    for k, route in ((30, "scan"), (100, "wide")):
        nn = NN_Wrapper(X, k)
        idx, dist = nn.get_nns(Q)
        assert nn.last_route == route, nn.last_route
        out.update({f"get_nns/k{k}/idx": ints(idx), f"get_nns/k{k}/dist": bits(dist)})
    return out


GROUPS = {"scan_f32": scan_f32, "scan_wide": scan_wide, "scan_long": scan_long, "cells": cells, "cells_wide": cells_wide,
          "cells_block": cells_block, "grid": grid, "wrapper": wrapper}


def record():
    """Every group's arrays under "<group>:<case>/<array>" (what the golden file holds)."""
    return {f"{group}:{key}": val for group, fn in GROUPS.items() for key, val in fn().items()}


@functools.lru_cache(maxsize=None)
def golden():
    with np.load(GOLDEN) as z:
        return {key: z[key] for key in z.files}


@pytest.mark.parametrize("group", list(GROUPS))
def test_entries_return_the_recorded_bits(group):
    got = GROUPS[group]()
    want = {key.split(":", 1)[1]: val for key, val in golden().items() if key.startswith(group + ":")}
    assert sorted(got) == sorted(want)
    for key in sorted(got):
        assert got[key].dtype == want[key].dtype == np.int32 and got[key].shape == want[key].shape, key
        differ = np.argwhere(got[key] != want[key])
        assert len(differ) == 0, (key, len(differ), differ[:4].tolist())
