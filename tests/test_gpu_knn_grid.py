"""GPU: the exact grid search, NN_Wrapper(..., algorithm="grid") -- the walk kernel (mgp_knn_grid_scan) and the route
through it against fp64 brute force over the whole table, and its shell counts against the numpy restatement of
tests/knn_grid_cases.py (pinned on the CPU by tests/test_knn_grid_cpu.py).

The comparison rule is the project's own (tests/test_gpu_neighbors_cells.py): position by position; a mismatch is
excused only between candidates whose fp64 distances differ by at most (2 + sqrt(d) / 2) ulp of fp32, and at most 0.2 %
of the entries may be excused.  The lattice compares sorted distances (mass ties leave positions undefined)."""

import numpy as np
import pytest

from tests import knn_grid_cases as G
from tests.util import to_dev

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


def wrapper(X, k, **kwargs):
    from muygpys_amd.neighbors import NN_Wrapper

    return NN_Wrapper(to_dev(X), k, algorithm="grid", **kwargs)


def index_of(nn):
    """The wrapper's own index as the restatement's: the same stored table, cells and edges, bit for bit."""
    edges = [np.empty(0, np.float32) if e is None else e.cpu().numpy() for e in nn._edges]
    return G.Index(nn.train.cpu().numpy(), nn._perm.cpu().numpy(), nn.cell_start.cpu().numpy(), tuple(nn.grid_shape), edges,
                   nn._mean.cpu().numpy())


def check_index(nn, n):
    dims = nn.grid_shape
    cs, perm = nn.cell_start.cpu().numpy(), nn._perm.cpu().numpy()
    assert len(dims) == 3 and cs.shape == (dims[0] * dims[1] * dims[2] + 1,) and cs[0] == 0 and cs[-1] == n
    assert (np.diff(cs) >= 0).all() and np.array_equal(np.sort(perm), np.arange(n))
    stored = G.linear(G.cells_of(nn.train.cpu().numpy(), index_of(nn).edges), dims)
    assert np.array_equal(stored, np.repeat(np.arange(len(cs) - 1), np.diff(cs)))  # every row sits in its own cell


def raw_scan(nn, q, k, self_pos=None, qcell=None):
    """mgp_knn_grid_scan itself on centred, padded queries (m, 4), every output pre-filled with a sentinel:
    (best_d, best_i (stored positions), shells)."""
    from muygpys_amd import _lib
    from muygpys_amd.neighbors import grid_cells

    q = to_dev(q, torch.float32).contiguous()
    m = q.shape[0]
    qcell = grid_cells(q, nn._edges).contiguous() if qcell is None else to_dev(qcell).to(torch.int32).contiguous()
    self_pos = None if self_pos is None else to_dev(self_pos).to(torch.int64).contiguous()
    best_d = torch.full((m, k), -7.0, device="cuda")
    best_i = torch.full((m, k), -7, device="cuda", dtype=torch.int32)
    shells = torch.full((m,), -7, device="cuda", dtype=torch.int32)
    g0, g1, g2 = nn.grid_shape
    rc = _lib.load().mgp_knn_grid_scan(_lib.ptr(nn.train), nn.train_count, _lib.ptr(nn.cell_start), g0, g1, g2,
                                       _lib.ptr(nn._edges_flat), _lib.ptr(q), m, _lib.ptr(qcell), _lib.ptr(self_pos), k,
                                       _lib.ptr(best_d), _lib.ptr(best_i), _lib.ptr(shells), _lib.stream_ptr())
    assert rc == 0
    torch.cuda.synchronize()
    return best_d.cpu().numpy(), best_i.cpu().numpy(), shells.cpu().numpy()


# ---- 1: the route ------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("d", [1, 2, 3])
@pytest.mark.parametrize("k", [1, 30, 64])
def test_route(d, k):
    """Fails before the route existed: the keyword was swallowed and the default scan answered (the answers alone
    would pass there; last_route, last_shells and the bound symbol would not)."""
    from muygpys_amd import _lib

    rng = np.random.default_rng(100 * d + k)
    n = 9001
    X = G.mirrored(rng.random((n // 2, d), dtype=G.F), 1.0, 0.5, rng)
    Q = rng.random((300, d), dtype=G.F)
    bi = rng.choice(n, size=300, replace=False)
    nn = wrapper(X[:, 0] if d == 1 else X, k)
    assert hasattr(_lib.load(), "mgp_knn_grid_scan")
    assert nn.algorithm == "grid" and nn.nn_method == "exact" and nn.train.shape == (n, 4) and nn.feature_count == d
    check_index(nn, n)
    for pts, rows, (idx, dist) in ((Q, None, nn.get_nns(to_dev(Q[:, 0] if d == 1 else Q))), (X[bi], bi, nn.get_batch_nns(to_dev(bi)))):
        assert nn.last_route == "grid"
        assert nn.last_shells.dtype == torch.int32 and nn.last_shells.shape == (300,) and nn.last_shells.is_cuda
        assert idx.dtype == torch.int64 and idx.shape == (300, k) and dist.dtype == torch.float32 and dist.shape == (300, k)
        idx, dist = idx.cpu().numpy(), dist.cpu().numpy()
        G.assert_same_neighbours(pts, X, idx, G.exact_neighbours(pts, X, k, rows), d, f"d={d} k={k}")
        ref = ((pts[:, None, :].astype(np.float64) - X[idx].astype(np.float64)) ** 2).sum(-1)
        np.testing.assert_allclose(dist, ref, rtol=1e-5, atol=1e-12)  # (exact centring: the sum's own rounding only)
        assert (dist[:, 1:] >= dist[:, :-1]).all()
        assert 0 <= int(nn.last_shells.min()) and int(nn.last_shells.max()) <= max(nn.grid_shape) - 1
        if rows is not None:
            assert not (idx == rows[:, None]).any()
    # every other value of the keyword is ignored as before, and the default route does not change
    other = type(nn)(to_dev(X), k, algorithm="kd_tree")
    other.get_nns(to_dev(Q))
    assert other.algorithm is None and other.last_route == "scan"


# ---- the shared cases: answers, and (7) a walk that stops as early as the restatement's ----------------------------------


@pytest.mark.parametrize("case", G.CASES, ids=[c.name for c in G.CASES])
def test_shared_cases_against_fp64_and_the_restated_walk(case):
    X, Q, rows, want = G.case_data(case)
    nn = wrapper(X, case.k, cell_rows=case.cell_rows, edges=case.edges)
    check_index(nn, case.n)
    idx, dist = nn.get_nns(to_dev(Q)) if rows is None else nn.get_batch_nns(to_dev(rows))
    got, shells = idx.cpu().numpy(), nn.last_shells.cpu().numpy()
    _, _, restated, scanned = G.search(index_of(nn), Q, case.k, rows)
    print(f"{case.name}: grid {nn.grid_shape}, shells mean {shells.mean():.2f} max {shells.max()} "
          f"(restated mean {restated.mean():.2f} max {restated.max()}), rows scanned per query {scanned.mean():.0f}")
    if case.kind == "lattice":
        G.assert_same_distances(Q, X, got, want, case.name)
    else:
        G.assert_same_neighbours(Q, X, got, want, case.d, case.name)
    if rows is not None:
        assert not (got == rows[:, None]).any()
    assert shells.max() <= max(nn.grid_shape) - 1
    # exact, and never a walk that does not stop early: one shell of room for a borderline rounding of tau against the bound
    assert (shells <= restated + 1).all(), (shells - restated).max()


# ---- 2: the raw entry on hand-built grids ----------------------------------------------------------------------------------


def hand_built(d, k, seed=0):
    """Cells of CELL_LENGTHS rows along axis 0 (explicit edges at 1 .. 9: the cells are [j, j + 1), the outer two
    unbounded and empty), the same lengths in every grid row of a 3-row (d = 2) or 2 x 2-row (d = 3) grid."""
    rng = np.random.default_rng(50 * d + seed)
    other = {1: [], 2: [3], 3: [2, 2]}[d]
    cols, grid_rows = [], int(np.prod(other)) if other else 1
    x0 = np.concatenate([j + rng.uniform(0.1, 0.9, size=c) for j, c in enumerate(G.CELL_LENGTHS)])
    cols.append(np.tile(x0, grid_rows))
    for a, g in enumerate(other):
        reps = int(np.prod(other[:a])) if a else 1
        cols.append(np.repeat(np.tile(np.arange(g), grid_rows // (g * reps)), len(x0) * reps) + rng.uniform(0.1, 0.9, size=len(x0) * grid_rows))
    X = np.stack(cols, axis=1).astype(np.float32)
    X = X[rng.permutation(len(X))]
    edges = [torch.arange(1.0, 10.0)] + [torch.arange(1.0, float(g)) for g in other]
    nn = wrapper(X, k, edges=edges)
    assert tuple(nn.grid_shape) == (10, *other, *([1] * (3 - d)))
    assert np.diff(nn.cell_start.cpu().numpy()).tolist() == G.CELL_LENGTHS * grid_rows
    return nn, X, rng


@pytest.mark.parametrize("d", [1, 2, 3])
@pytest.mark.parametrize("m", [1, 3, 4, 5, 257])
def test_raw_entry_on_hand_built_grids(d, m):
    """The C entry against fp64 brute force over ITS inputs (the stored table, the centred queries): every slot of every
    output written, stored positions, the k nearest whatever the cell populations (0, 1, 63, 64, 65, 129, 1000 ...)."""
    k = 10
    nn, X, rng = hand_built(d, k)
    n, table = len(X), nn.train.cpu().numpy()
    q = np.zeros((m, 4), dtype=np.float32)
    q[:, :d] = rng.uniform(-1.0, 11.0, size=(m, d)).astype(np.float32) - nn._mean.cpu().numpy()
    bd, bi, shells = raw_scan(nn, q, k)
    assert (bi >= 0).all() and (bi < n).all() and (bd >= 0).all() and (shells >= 0).all() and (shells <= 9).all()
    order = np.stack([row[np.lexsort((row, dr))] for row, dr in zip(bi, bd)])  # (distance, then stored position)
    G.assert_same_neighbours(q, table, order.astype(np.int64), G.exact_neighbours(q, table, k), d, f"d={d} m={m}")
    ref = ((q[:, None, :].astype(np.float64) - table[bi].astype(np.float64)) ** 2).sum(-1)
    np.testing.assert_allclose(bd, ref, rtol=1e-6)
    # the restated walk on the same index: the same shells (no rounding is borderline on this table) -- and the same
    # lists whatever cell the caller claims for the query (the bound holds for any, the clamp keeps it inside the grid)
    index = index_of(nn)
    want = [G.walk(index, q[i], G.cells_of(q[i:i + 1], index.edges)[0], k) for i in range(m)]
    assert np.array_equal(shells, [w[2] for w in want])
    assert np.array_equal(np.sort(bi, axis=1), np.sort([w[0] for w in want], axis=1))
    wild = rng.integers(-5, 15, size=(m, 3))
    bd2, bi2, shells2 = raw_scan(nn, q, k, qcell=wild)
    assert np.array_equal(np.sort(bi2, axis=1), np.sort(bi, axis=1)) and (shells2 <= 9).all()
    # self-exclusion by stored position
    pos = rng.integers(0, n, size=m)
    qs = table[pos]
    _, bi3, _ = raw_scan(nn, qs, k, self_pos=pos)
    assert not (bi3 == pos[:, None]).any()
    mine = np.stack([row[np.lexsort((row, sq))] for row, sq in zip(bi3, ((qs[:, None, :].astype(np.float64) - table[bi3]) ** 2).sum(-1))])
    G.assert_same_neighbours(qs, table, mine.astype(np.int64), G.exact_neighbours(qs, table, k, pos), d, "self")


# ---- 3: queries on an edge, on the corner, outside the box ---------------------------------------------------------------


@pytest.mark.parametrize("d", [1, 2, 3])
def test_queries_on_edges_corners_and_outside(d):
    rng = np.random.default_rng(30 + d)
    n, k = 6001, 20
    X = G.mirrored(rng.random((n // 2, d), dtype=G.F), 1.0, 0.5, rng)
    edges = [torch.arange(1, 8) / 8.0 for _ in range(d)]  # (dyadic: the centred edges are exact, a query can sit ON one)
    nn = wrapper(X, k, edges=edges)
    assert tuple(nn.grid_shape) == (8,) * d + (1,) * (3 - d)
    # on interior edges, on the box's corners (not at 0.5: the centre of the table's symmetry ties every mirrored pair)
    pts = [np.full(d, 0.25), np.full(d, 0.625), np.zeros(d), np.ones(d), np.full(d, 0.875)]
    for a in range(d):
        for v in (-0.25, 1.25, -1.0, 2.0):  # outside on each side of each axis; one box width away
            p = np.full(d, 0.375)
            p[a] = v
            pts.append(p)
    pts.append(np.full(d, 2.0))
    pts.append(np.full(d, -1.0))
    Q = np.array(pts, dtype=np.float32)
    got = nn.get_nns(to_dev(Q))[0].cpu().numpy()
    shells = nn.last_shells.cpu().numpy()
    G.assert_same_neighbours(Q, X, got, G.exact_neighbours(Q, X, k), d, f"d={d}")
    assert (shells <= 7).all()
    _, _, restated, _ = G.search(index_of(nn), Q, k)
    assert (shells <= restated + 1).all()
    # a query ON an edge belongs to the upper cell, like a row
    from muygpys_amd.neighbors import grid_cells

    on = torch.zeros((1, 4), device="cuda")
    on[0, :d] = 0.25 - 0.5
    assert grid_cells(on, nn._edges)[0, :d].tolist() == [2] * d


# ---- 4: the walk must widen --------------------------------------------------------------------------------------------


def test_walk_widens_between_two_clusters():
    rng = np.random.default_rng(41)
    half = (rng.integers(0, 2**20, (400, 2)) / 2.0**24).astype(G.F)  # [0, 1/16)^2 and its mirror image
    X = G.mirrored(half, 1.0, None, rng)
    nn = wrapper(X, 10, cell_rows=8)
    Q = np.array([[0.5, 0.375], [0.25, 0.75], [0.5, 0.0]], dtype=G.F)
    got = nn.get_nns(to_dev(Q))[0].cpu().numpy()
    shells = nn.last_shells.cpu().numpy()
    G.assert_same_neighbours(Q, X, got, G.exact_neighbours(Q, X, 10), 2)
    _, _, restated, _ = G.search(index_of(nn), Q, 10)
    assert shells.min() >= 3 and np.array_equal(shells, restated)


@pytest.mark.parametrize("d", [1, 2, 3])
def test_k_beyond_the_block_and_every_other_row(d):
    """k = 64 at two rows per cell (the 3^d block holds 6 to 54); then n = k + 1 with batch queries: every answer is all
    other rows and the walk reaches the grid's edge."""
    rng = np.random.default_rng(42 + d)
    X = G.mirrored(rng.random((500, d), dtype=G.F), 1.0, 0.5, rng)
    nn = wrapper(X, 64, cell_rows=2)
    # (not the row at the centre of the table's symmetry: as a query it ties every mirrored pair exactly)
    bi = rng.choice(np.flatnonzero((X != 0.5).any(1)), size=200, replace=False)
    got = nn.get_batch_nns(to_dev(bi))[0].cpu().numpy()
    G.assert_same_neighbours(X[bi], X, got, G.exact_neighbours(X[bi], X, 64, bi), d)
    assert int(nn.last_shells.min()) >= (2 if d < 3 else 1)
    X = G.mirrored(rng.random((32, d), dtype=G.F), 1.0, 0.5, rng)  # n = 65
    nn = wrapper(X, 64, cell_rows=2)
    rows = np.arange(65)
    got = nn.get_batch_nns(to_dev(rows))[0].cpu().numpy()
    assert all(sorted(got[r].tolist()) == sorted(set(range(65)) - {r}) for r in rows)
    index = index_of(nn)
    cells = G.cells_of(index.x, index.edges)[np.argsort(index.perm)]
    reach = np.max([np.maximum(cells[:, a], index.dims[a] - 1 - cells[:, a]) for a in range(3)], axis=0)
    assert np.array_equal(nn.last_shells.cpu().numpy(), reach)
    with pytest.raises(ValueError, match=r"can give 63 \(n = 64"):
        wrapper(X[:64], 64).get_batch_nns(to_dev(rows[:3]))  # (k > n - 1 for batch queries)
    with pytest.raises(ValueError, match=r"can give 63 \(n = 63"):
        wrapper(X[:63], 64).get_nns(to_dev(X[:3]))           # (k > n)


# ---- 5: duplicates ---------------------------------------------------------------------------------------------------------


def test_batch_queries_return_a_duplicate_but_never_themselves():
    rng = np.random.default_rng(51)
    n, d, k = 6001, 2, 10
    X = rng.random((n, d), dtype=G.F)
    bi = rng.choice(n - 100, size=100, replace=False)
    copies = np.arange(n - 100, n)[rng.permutation(100)]
    X[copies[:60]] = X[bi[:60]]  # (60 of the 100 batch rows have a twin)
    nn = wrapper(X, k)
    idx, dist = nn.get_batch_nns(to_dev(bi))
    idx, dist = idx.cpu().numpy(), dist.cpu().numpy()
    assert not (idx == bi[:, None]).any()
    assert np.array_equal(idx[:60, 0], copies[:60]) and (dist[:60, 0] == 0).all()
    assert (dist[60:, 0] > 0).all() and (dist[:, 1] > 0).all()
    idx2, dist2 = nn.get_batch_nns(to_dev(copies[:60]))
    assert np.array_equal(idx2.cpu().numpy()[:, 0], bi[:60]) and (dist2.cpu().numpy()[:, 0] == 0).all()


def test_lattice_answers_do_not_depend_on_the_query_order():
    case = next(c for c in G.CASES if c.kind == "lattice")
    X, Q, rows, want = G.case_data(case)
    nn = wrapper(X, case.k)
    idx, dist = nn.get_batch_nns(to_dev(rows))
    shells = nn.last_shells.clone()
    order = np.random.default_rng(52).permutation(len(rows))
    idx2, dist2 = nn.get_batch_nns(to_dev(rows[order]))
    assert torch.equal(idx2, idx[to_dev(order)]) and torch.equal(dist2, dist[to_dev(order)])  # bit for bit
    assert torch.equal(nn.last_shells, shells[to_dev(order)])
    dist = dist.cpu().numpy()
    assert (dist == np.round(dist)).all() and (dist[:, :11] == 0).sum() > 0  # integer distances, the copies first


# ---- 6: a constant column ------------------------------------------------------------------------------------------------


def test_constant_column_in_the_middle():
    rng = np.random.default_rng(61)
    n, k = 9001, 30
    X = G.mirrored(rng.random((n // 2, 3), dtype=G.F), 1.0, 0.5, rng)
    X[:, 1] = 0.75
    nn = wrapper(X, k)
    assert nn.grid_shape[1] == 1 and nn.grid_shape[0] > 1 and nn.grid_shape[2] > 1 and nn._edges[1].numel() == 0
    check_index(nn, n)
    bi = rng.choice(n, size=300, replace=False)
    got = nn.get_batch_nns(to_dev(bi))[0].cpu().numpy()
    G.assert_same_neighbours(X[bi], X, got, G.exact_neighbours(X[bi], X, k, bi), 3)
    assert int(nn.last_shells.max()) <= 2
    Q = rng.random((100, 3), dtype=G.F)  # (off the plane of the table: the axis of one cell still counts in the distance)
    got = nn.get_nns(to_dev(Q))[0].cpu().numpy()
    G.assert_same_neighbours(Q, X, got, G.exact_neighbours(Q, X, k), 3)


# ---- a query that is at no distance from anything ------------------------------------------------------------------------


def test_nan_query_is_flagged_and_a_refused_search_leaves_the_record():
    rng = np.random.default_rng(71)
    X = G.mirrored(rng.random((1500, 2), dtype=G.F), 1.0, 0.5, rng)
    nn = wrapper(X, 10)
    Q = rng.random((9, 2), dtype=G.F)
    Q[4, 1] = np.nan
    idx, dist = nn.get_nns(to_dev(Q))
    assert nn.last_short.dtype == torch.int32 and nn.last_short.cpu().tolist() == [0, 0, 0, 0, 1, 0, 0, 0, 0]
    shells = nn.last_shells.cpu().numpy()
    assert shells.max() <= max(nn.grid_shape) - 1  # (the NaN query's walk ends at the grid's edge, not later)
    assert torch.isnan(dist[4]).all() and bool((idx[4] == nn._perm[0]).all()) and bool(torch.isfinite(dist[[0, 8]]).all())
    keep = np.arange(9) != 4
    G.assert_same_neighbours(Q[keep], X, idx.cpu().numpy()[keep], G.exact_neighbours(Q[keep], X, 10), 2)
    # a search the route refuses does not overwrite what the last served one left
    before = nn.last_shells
    with pytest.raises(ValueError, match="k <= 64"):
        nn._get_nns(to_dev(Q), 65)
    assert nn.last_shells is before
