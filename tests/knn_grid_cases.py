"""The exact grid search (NN_Wrapper(..., algorithm="grid"), csrc/mgp_knn_grid.hip) restated in numpy, and the cases the
CPU and the GPU test share.

The restatement is the yardstick of the kernel's WALK: the same layout (centred table, cells by comparison against the
stored edges, linear id with axis 0 fastest), the same shells, the same fp32 difference-form distances
((s0 + s1) + (s2 + s3), one rounding per operation -- numpy's float32 arithmetic is the kernel's), the same bound
tau < t^2 (1 - 2^-20) on every face with cells left, the same tie rule (distance, then stored position).  It returns
neighbours and the radius of the last shell.  tests/test_knn_grid_cpu.py pins it against fp64 brute force.

The tables.  The index centres the table on its fp32 mean before anything is measured, and at d <= 3 a neighbour's
squared distance is tiny next to a coordinate (n = 20 000 uniform rows in the unit square, k = 30: r^2 ~ 5e-4): one
rounding of a centred coordinate (2^-26) moves such a distance by 2 r 2^-26 ~ 1e-9, twenty of its own units of
roundoff, which the project's tie rule ((2 + sqrt(d) / 2) ulp of the squared distance) does not and should not excuse.
So every table here centres EXACTLY: its rows come in mirrored pairs x, c - x on a dyadic lattice (multiples of 2^-24
in [0, 1], which is what numpy's float32 generator draws; integers for the lattice table), the fp64 mean is c / 2 bit
for bit, and x - c / 2 is representable.  Queries are drawn on the same lattice (2^-22 where they leave the box).
fp32 against fp64 then differs by the rounding of the sum of squares alone, which is what the tie rule is about.
"""

import functools
from dataclasses import dataclass

import numpy as np

SLACK = np.float32(1.0) - np.float32(2.0**-20)
F = np.float32


# ---- the index ---------------------------------------------------------------------------------------------------------


@dataclass
class Index:
    x: np.ndarray           # (n, 4) float32: the stored table, centred and zero-padded, cell by cell
    perm: np.ndarray        # stored position -> caller's row
    cell_start: np.ndarray  # (g0 g1 g2 + 1) int64
    dims: tuple             # (g0, g1, g2)
    edges: list             # three float32 arrays of g_a - 1 interior edges (centred coordinates)
    mean: np.ndarray        # (d) float32


def cells_of(x, edges):
    """(m, 3) cells per axis: c_a = #{j : E_a[j] <= x_a}."""
    out = np.zeros((len(x), 3), dtype=np.int64)
    for a, e in enumerate(edges):
        if len(e):
            out[:, a] = np.searchsorted(e, x[:, a], side="right")
    return out


def linear(cells, dims):
    return cells[:, 0] + dims[0] * (cells[:, 1] + dims[1] * cells[:, 2])


def uniform_edges(x, d, cell_rows):
    """The bounding box in equal parts, g_a from the project's grid_dims (a pure function; its own invariants are in
    tests/test_knn_grid_cpu.py)."""
    from muygpys_amd.neighbors import grid_dims

    lo, hi = x[:, :d].min(0).astype(np.float64), x[:, :d].max(0).astype(np.float64)
    dims = grid_dims(len(x), (hi - lo).tolist(), cell_rows)
    edges = [(lo[a] + np.arange(1, dims[a]) * ((hi[a] - lo[a]) / dims[a])).astype(F) for a in range(d)]
    return edges + [np.empty(0, F)] * (3 - d)


def quantile_edges(x, d, cell_rows):
    from muygpys_amd.neighbors import grid_dims

    lo, hi = x[:, :d].min(0).astype(np.float64), x[:, :d].max(0).astype(np.float64)
    dims = grid_dims(len(x), (hi - lo).tolist(), cell_rows)
    n = len(x)
    edges = [np.sort(x[:, a])[(np.arange(1, dims[a]) * n) // dims[a]] for a in range(d)]
    return edges + [np.empty(0, F)] * (3 - d)


def make_index(X, cell_rows=32, edges="uniform"):
    """The index of a float32 table (n, d); ``edges``: "uniform", "quantile" or d arrays in the table's coordinates."""
    X = np.asarray(X, dtype=F).reshape(len(X), -1)
    n, d = X.shape
    mean = X.astype(np.float64).mean(0).astype(F)
    x = np.zeros((n, 4), dtype=F)
    x[:, :d] = X - mean
    if isinstance(edges, str):
        e = (uniform_edges if edges == "uniform" else quantile_edges)(x, d, cell_rows)
    else:
        e = [np.asarray(v, dtype=F) - mean[a] for a, v in enumerate(edges)] + [np.empty(0, F)] * (3 - d)
    dims = tuple(len(v) + 1 for v in e)
    cell = linear(cells_of(x, e), dims)
    perm = np.argsort(cell, kind="stable")
    cell_start = np.concatenate([[0], np.cumsum(np.bincount(cell, minlength=dims[0] * dims[1] * dims[2]))]).astype(np.int64)
    return Index(x[perm], perm, cell_start, dims, e, mean)


# ---- the walk ----------------------------------------------------------------------------------------------------------


def shell_runs(c, sh, dims):
    """The runs of shell ``sh`` around cell ``c``: (first cell, last cell) in linear ids, each one grid row's piece."""
    g0, g1, g2 = dims
    l = [max(c[a] - sh, 0) for a in range(3)]
    h = [min(c[a] + sh, dims[a] - 1) for a in range(3)]
    runs = []
    for j2 in range(l[2], h[2] + 1):
        for j1 in range(l[1], h[1] + 1):
            row = (j2 * g1 + j1) * g0
            if max(abs(j1 - c[1]), abs(j2 - c[2])) == sh:
                runs.append((row + l[0], row + h[0]))
            else:
                if c[0] - sh >= 0:
                    runs.append((row + c[0] - sh, row + c[0] - sh))
                if c[0] + sh <= g0 - 1:
                    runs.append((row + c[0] + sh, row + c[0] + sh))
    return runs, l, h


def fp32_dists(q, rows):
    e = q[None, :] - rows  # float32 throughout
    s = e * e
    return (s[:, 0] + s[:, 1]) + (s[:, 2] + s[:, 3])


def walk(index, q, c, k, self_pos=None):
    """One query (centred, padded float32 (4,)) from cell ``c``: (stored positions of the k nearest by (fp32 distance,
    position), their fp32 distances, the radius of the last shell, rows scanned)."""
    q = np.asarray(q, dtype=F)
    pos, dist = np.empty(0, np.int64), np.empty(0, F)
    gmax, sh, scanned = max(index.dims), 0, 0
    while True:
        runs, l, h = shell_runs(c, sh, index.dims)
        for first, last in runs:
            r, e = index.cell_start[first], index.cell_start[last + 1]
            if e > r:
                rows = np.arange(r, e)
                dd = fp32_dists(q, index.x[r:e])
                keep = ~np.isnan(dd) & (rows != (-1 if self_pos is None else self_pos))
                pos, dist = np.concatenate([pos, rows[keep]]), np.concatenate([dist, dd[keep]])
                scanned += e - r
        order = np.lexsort((pos, dist))[:k]
        pos, dist = pos[order], dist[order]
        tau = dist[-1] if len(dist) >= k else F(np.inf)
        open_, done = False, True
        for a in range(3):
            if l[a] > 0:
                t = q[a] - index.edges[a][l[a] - 1]
                open_, done = True, done and bool(t > 0 and tau < (t * t) * SLACK)
            if h[a] < index.dims[a] - 1:
                t = index.edges[a][h[a]] - q[a]
                open_, done = True, done and bool(t > 0 and tau < (t * t) * SLACK)
        if not open_ or done or sh + 1 >= gmax:
            return pos, dist, sh, scanned
        sh += 1


def search(index, Q, k, self_rows=None):
    """Queries in the table's coordinates (m, d) float32: (rows (m, k) in the caller's numbering, ascending by (fp32
    distance, stored position), fp32 distances, shells (m), rows scanned (m))."""
    Q = np.asarray(Q, dtype=F).reshape(len(Q), -1)
    d = Q.shape[1]
    q = np.zeros((len(Q), 4), dtype=F)
    q[:, :d] = Q - index.mean
    cells = cells_of(q, index.edges)
    inv = np.empty_like(index.perm)
    inv[index.perm] = np.arange(len(index.perm))
    rows = np.empty((len(Q), k), dtype=np.int64)
    dist = np.empty((len(Q), k), dtype=F)
    shells, scanned = np.empty(len(Q), dtype=np.int64), np.empty(len(Q), dtype=np.int64)
    for i in range(len(Q)):
        p, dd, shells[i], scanned[i] = walk(index, q[i], cells[i], k, None if self_rows is None else inv[self_rows[i]])
        assert len(p) == k, (i, len(p))
        rows[i], dist[i] = index.perm[p], dd
    return rows, dist, shells, scanned


# ---- the reference and the comparison rule -----------------------------------------------------------------------------


def sq_dists(pt, rows):
    return ((rows.astype(np.float64) - pt.astype(np.float64)) ** 2).sum(1)


def exact_neighbours(pts, X, k, self_rows=None):
    """fp64 brute force over the whole table, ascending (ties: row number)."""
    X = X.reshape(len(X), -1)
    pts = pts.reshape(len(pts), -1)
    want = np.empty((len(pts), k), dtype=np.int64)
    for r in range(len(pts)):
        dd = sq_dists(pts[r], X)
        if self_rows is not None:
            dd[self_rows[r]] = np.inf
        want[r] = np.argsort(dd, kind="stable")[:k]
    return want


def assert_same_neighbours(pts, X, got, want, d, what=""):
    """The project's rule (tests/test_gpu_neighbors_cells.py): position by position; a mismatch only between candidates
    whose fp64 distances differ by at most (2 + sqrt(d) / 2) ulp of fp32, 0.2 % of the entries at most."""
    X, pts = X.reshape(len(X), -1), pts.reshape(len(pts), -1)
    assert got.shape == want.shape, (got.shape, want.shape)
    diff = np.argwhere(got != want)
    print(f"{what}: {len(diff)} of {got.size} positions differ from fp64 brute force")
    for r, c in diff:
        assert 0 <= got[r, c] < len(X), (what, r, c, got[r, c])
        da = sq_dists(pts[r], X[got[r, c]][None])[0]
        db = sq_dists(pts[r], X[want[r, c]][None])[0]
        assert abs(da - db) <= (2 + 0.5 * np.sqrt(d)) * np.spacing(np.float32(max(da, db))), (what, r, c, da, db)
    assert len(diff) <= 0.002 * got.size, (what, len(diff), got.size)
    for row in got:
        assert len(set(row.tolist())) == len(row), what


def assert_same_distances(pts, X, got, want, what=""):
    """Mass ties (the lattice): position-level equality is undefined; the sorted fp64 distances of the returned rows
    are those of the reference, so every returned row is at most at the k-th distance and none is missing below it."""
    X, pts = X.reshape(len(X), -1), pts.reshape(len(pts), -1)
    for r in range(len(pts)):
        assert len(set(got[r].tolist())) == got.shape[1], (what, r)
        da, db = np.sort(sq_dists(pts[r], X[got[r]])), np.sort(sq_dists(pts[r], X[want[r]]))
        assert (da <= db[-1]).all() and np.array_equal(da, db), (what, r)


# ---- the tables --------------------------------------------------------------------------------------------------------


def mirrored(half, centre_sum, odd_row=None, rng=None):
    """x and centre_sum - x for every row of ``half`` (+ the centre itself for an odd count), shuffled: the fp64 mean is
    centre_sum / 2 exactly (see the module docstring)."""
    parts = [half, (F(centre_sum) - half).astype(F)]
    if odd_row is not None:
        parts.append(np.full((1, half.shape[1]), odd_row, dtype=F))
    X = np.concatenate(parts)
    return X[rng.permutation(len(X))]


@dataclass(frozen=True)
class Case:
    name: str
    kind: str        # "uniform" | "mixture" | "lattice" | "outside"
    n: int
    d: int
    k: int
    cell_rows: int = 32
    edges: str = "uniform"
    batch: bool = True   # batch queries (self-exclusion) or 200 free queries
    seed: int = 0


CASES = [
    Case("uniform d=2 k=30 rows/cell=16", "uniform", 20001, 2, 30, 16),
    Case("uniform d=2 k=30 rows/cell=32", "uniform", 20001, 2, 30, 32),
    Case("uniform d=3 k=30 rows/cell=16", "uniform", 20001, 3, 30, 16),
    Case("uniform d=3 k=30 rows/cell=32", "uniform", 20001, 3, 30, 32),
    Case("uniform d=1 k=64 rows/cell=32", "uniform", 20001, 1, 64, 32),
    Case("30-cluster mixture d=2 k=30", "mixture", 21002, 2, 30, 32),
    Case("30-cluster mixture d=2 k=30 quantile edges", "mixture", 21002, 2, 30, 32, "quantile"),
    Case("integer lattice 40 x 40 with duplicates", "lattice", 20002, 2, 30, 32),
    Case("queries up to one box width outside", "outside", 20001, 2, 30, 32, "uniform", False),
]
UNIFORM = [c for c in CASES if c.kind == "uniform"]
QUERIES = 300


@functools.lru_cache(maxsize=None)
def case_data(case):
    """(X (n, d) float32, Q (m, d) float32, self_rows (m) or None, want (m, k) fp64 brute force) -- computed once,
    read-only."""
    rng = np.random.default_rng(7000 + 10 * CASES.index(case) + case.seed)
    n, d = case.n, case.d
    if case.kind in ("uniform", "outside"):
        X = mirrored(rng.random((n // 2, d), dtype=F), 1.0, 0.5 if n % 2 else None, rng)
    elif case.kind == "mixture":  # 15 centres and their mirror images, sigma = 0.02, on the 2^-24 lattice, clipped
        centres = rng.random((15, d)) * 0.8 + 0.1
        pts = centres[rng.integers(0, 15, n // 2)] + 0.02 * rng.normal(size=(n // 2, d))
        half = (np.round(np.clip(pts, 0.0, 1.0) * 2.0**24) / 2.0**24).astype(F)
        X = mirrored(half, 1.0, 0.5 if n % 2 else None, rng)
    else:  # the lattice: 1 600 points, ~12 copies each
        X = mirrored(rng.integers(0, 40, (n // 2, d)).astype(F), 39.0, None, rng)
    assert len(X) == n and n % 64
    if case.batch:
        rows = rng.choice(n, size=QUERIES, replace=False)
        Q = X[rows]
    else:  # every side of every axis, up to one box width away, on the 2^-22 lattice
        rows = None
        Q = (rng.integers(-(2**22), 2 * 2**22, (200, d)) / 2.0**22).astype(F)
        Q[:4] = [[-1.0, 0.5], [2.0, 0.5], [0.5, -1.0], [0.5, 2.0]]
    want = exact_neighbours(Q, X, case.k, rows)
    for a in (X, Q, want) + (() if rows is None else (rows,)):
        a.setflags(write=False)
    return X, Q, rows, want


# the hand-built 1-D cell populations of the raw-entry test: the 64-lane step boundaries, empty cells first and last
CELL_LENGTHS = [0, 1, 63, 64, 65, 0, 129, 1000, 200, 0]
