"""GPU: the inverted-cell (IVF) neighbour search, nn_method="ivf" -- the cell scan kernel (mgp_knn_cells_scan) against
fp64 brute force over its own candidate set, the index against its defining properties, and the search at
nprobe == nlist against scikit-learn's exact neighbours (the reference's CPU implementation, neighbors.py:106-107,242).

Where two candidates at a position differ, the project's tie rule (tests/test_gpu_neighbors.py) decides: their fp64
distances from the query may differ by at most (2 + sqrt(d) / 2) ulp of fp32 -- the rounding of a d-term sum of squares
-- and at most 0.2 % of the entries may be excused that way."""

import functools

import numpy as np
import pytest

from tests.util import to_dev

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

CELL_LENGTHS = [0, 1, 63, 64, 65, 0, 129, 1000, 200, 0]  # the 64-lane step boundaries; empty cells, first and last too


def sq_dists(pt, rows):
    return ((rows.astype(np.float64) - pt.astype(np.float64)) ** 2).sum(1)


def assert_same_neighbours(pts, X, got, want, d, what=""):
    """Position by position; a mismatch only between candidates tied to fp32 rounding, 0.2 % of the entries at most."""
    assert got.shape == want.shape, (got.shape, want.shape)
    diff = np.argwhere(got != want)
    for r, c in diff:
        assert 0 <= got[r, c] < len(X), (what, r, c, got[r, c])
        da = sq_dists(pts[r], X[got[r, c]][None])[0]
        db = sq_dists(pts[r], X[want[r, c]][None])[0]
        assert abs(da - db) <= (2 + 0.5 * np.sqrt(d)) * np.spacing(np.float32(max(da, db))), (what, r, c, da, db)
    assert len(diff) <= 0.002 * got.size, (what, len(diff), got.size)
    for row in got:
        assert len(set(row.tolist())) == len(row), what


def exact_neighbours(pts, X, k, self_rows=None):
    """fp64 brute force over the whole table, ascending (ties: row number)."""
    want = np.empty((len(pts), k), dtype=np.int64)
    for r in range(len(pts)):
        dd = sq_dists(pts[r], X)
        if self_rows is not None:
            dd[self_rows[r]] = np.inf
        want[r] = np.argsort(dd, kind="stable")[:k]
    return want


def candidate_rows(nn, probes_row, self_row=None):
    cs, perm = nn.cell_start.cpu().numpy(), nn._perm.cpu().numpy()
    cand = np.concatenate([perm[cs[c]:cs[c + 1]] for c in probes_row] + [np.empty(0, dtype=np.int64)])
    return cand if self_row is None else cand[cand != self_row]


def restated_search(nn, pts, X, k, self_rows=None, probes=None):
    """What the probed search must return, in fp64 numpy: per query the k nearest among the rows of probe(q)'s cells
    -- over the whole table where those hold fewer than k (the flagged queries).  Returns (rows (m, k), short (m))."""
    if probes is None:
        probes = nn.probe(to_dev(pts, torch.float32)).cpu().numpy()
    want = np.empty((len(pts), k), dtype=np.int64)
    short = np.zeros(len(pts), dtype=bool)
    for r in range(len(pts)):
        me = None if self_rows is None else self_rows[r]
        cand = candidate_rows(nn, probes[r], me)
        short[r] = len(cand) < k
        if short[r]:
            cand = np.arange(len(X)) if me is None else np.delete(np.arange(len(X)), me)
        dd = sq_dists(pts[r], X[cand])
        want[r] = cand[np.lexsort((cand, dd))[:k]]
    return want, short


def raw_scan(nn, pts, probes, k, self_rows=None):
    """mgp_knn_cells_scan itself on the index's stored table: (best_d, best_i (stored positions), short_flag)."""
    from muygpys_amd import _lib

    q = nn._pad_features(to_dev(pts, torch.float32) - nn._mean)
    m = q.shape[0]
    probes = probes.to(torch.int32).contiguous()
    self_pos = None if self_rows is None else nn._inv[to_dev(self_rows)].contiguous()
    best_d = torch.full((m, k), -7.0, device="cuda")
    best_i = torch.full((m, k), -7, device="cuda", dtype=torch.int32)
    short = torch.full((m,), -7, device="cuda", dtype=torch.int32)
    rc = _lib.load().mgp_knn_cells_scan(_lib.ptr(nn.train), nn.train_count, nn._width, _lib.ptr(nn.cell_start), nn.nlist,
                                        _lib.ptr(q), m, _lib.ptr(probes), probes.shape[1], _lib.ptr(self_pos), k,
                                        _lib.ptr(best_d), _lib.ptr(best_i), _lib.ptr(short), _lib.stream_ptr())
    assert rc == 0
    torch.cuda.synchronize()
    return best_d.cpu().numpy(), best_i.cpu().numpy(), short.cpu().numpy()


def hand_built(d, nprobe, k, seed=0):
    """An index over cells of CELL_LENGTHS rows, the rows dealt to the cells at random (a row need not sit in its nearest
    cell: the scan's candidate set is what the layout says, not what the geometry says)."""
    from muygpys_amd.neighbors import NN_Wrapper

    rng = np.random.default_rng(1000 * d + seed)
    n, nlist = sum(CELL_LENGTHS), len(CELL_LENGTHS)
    X = rng.normal(size=(n, d)).astype(np.float32)
    centroids = rng.normal(size=(nlist, d)).astype(np.float32)
    assignment = rng.permutation(np.repeat(np.arange(nlist), CELL_LENGTHS))
    nn = NN_Wrapper._from_cells(to_dev(X), k, to_dev(centroids), to_dev(assignment), nprobe=nprobe)
    assert nn.cell_start.cpu().tolist() == np.concatenate([[0], np.cumsum(CELL_LENGTHS)]).tolist()
    return nn, X, rng


def test_ivf_constructs_and_returns_true_distances():
    """Fails before the index existed (NotImplementedError): the search runs, and what it returns are rows of the table
    with their squared distances.  The bound: the difference form in fp32 on the centred table -- every coordinate
    carries a rounding of 2^-24 of its size, so a squared distance 2^-23 (|q| + |x|) / |q - x| + d 2^-24 of its own,
    ~2e-6 here; 1e-5 (+ 1e-6 absolute), the exact path's own bound in tests/test_gpu_neighbors.py."""
    from muygpys_amd.neighbors import NN_Wrapper

    rng = np.random.default_rng(0)
    X = rng.normal(size=(5000, 8)).astype(np.float32)
    Q = rng.normal(size=(300, 8)).astype(np.float32)
    nn = NN_Wrapper(to_dev(X), 10, nn_method="ivf")
    assert nn.nn_method == "ivf" and nn.nlist == 71 and nn.nprobe == 16
    idx, dist = nn.get_nns(to_dev(Q))
    assert idx.dtype == torch.int64 and idx.shape == (300, 10) and dist.shape == (300, 10) and dist.dtype == torch.float32
    idx, dist = idx.cpu().numpy(), dist.cpu().numpy()
    assert idx.min() >= 0 and idx.max() < 5000
    ref = ((Q[:, None, :].astype(np.float64) - X[idx].astype(np.float64)) ** 2).sum(-1)
    np.testing.assert_allclose(dist, ref, rtol=1e-5, atol=1e-6)
    assert (dist[:, 1:] >= dist[:, :-1]).all()
    with pytest.raises(NotImplementedError):
        NN_Wrapper(to_dev(X), 10, nn_method="hnsw")


@pytest.mark.parametrize("d,k,nprobe", [(4, 1, 1), (4, 1, 3), (8, 10, 3), (8, 50, 10), (8, 64, 1), (40, 10, 1), (40, 50, 3),
                                        (40, 1, 10), (64, 64, 10), (64, 64, 3), (64, 10, 1)])
def test_scan_returns_the_k_nearest_of_its_candidate_set(d, k, nprobe):
    """The kernel against fp64 brute force over the rows of the probed cells, through the wrapper (test and batch
    queries; a query with fewer than k candidates is answered exactly) and through the C entry (the raw lists: the
    same set whatever the order of the cells, -1 / +inf where candidates are missing)."""
    nn, X, rng = hand_built(d, nprobe, k)
    n = len(X)
    Q = rng.normal(size=(150, d)).astype(np.float32)
    bi = rng.choice(n, size=150, replace=False)
    want, short = restated_search(nn, Q, X, k)
    got = nn.get_nns(to_dev(Q))[0].cpu().numpy()
    assert np.array_equal(nn.last_short.cpu().numpy().astype(bool), short)
    assert_same_neighbours(Q, X, got, want, d, "test")
    want_b, short_b = restated_search(nn, X[bi], X, k, self_rows=bi)
    got_b = nn.get_batch_nns(to_dev(bi))[0].cpu().numpy()
    assert np.array_equal(nn.last_short.cpu().numpy().astype(bool), short_b)
    assert_same_neighbours(X[bi], X, got_b, want_b, d, "batch")
    assert not (got_b == bi[:, None]).any()

    # the C entry: cells in the probe order and reversed
    probes = nn.probe(to_dev(Q))
    perm = nn._perm.cpu().numpy()
    bd, bi_raw, flag = raw_scan(nn, Q, probes, k)
    bd2, bi2, flag2 = raw_scan(nn, Q, probes.flip(1), k)
    assert np.array_equal(np.sort(bi_raw, axis=1), np.sort(bi2, axis=1)) and np.array_equal(np.sort(bd, axis=1), np.sort(bd2, axis=1))
    assert np.array_equal(flag, short.astype(np.int32)) and np.array_equal(flag2, flag)
    probes = probes.cpu().numpy()
    rows = np.empty((len(Q), k), dtype=np.int64)
    full = np.empty_like(rows)
    for r in range(len(Q)):
        cand = candidate_rows(nn, probes[r])
        have = min(k, len(cand))
        assert (bi_raw[r] >= 0).sum() == have and np.isinf(bd[r][bi_raw[r] < 0]).all() and (bi_raw[r][bi_raw[r] < 0] == -1).all()
        mine = perm[bi_raw[r][bi_raw[r] >= 0]]
        assert len(set(mine.tolist())) == have and np.isin(mine, cand).all()
        order = np.lexsort((cand, sq_dists(Q[r], X[cand])))[:k]
        # (short lists padded with one row on both sides: the comparison below is over what the kernel did return)
        full[r] = np.concatenate([cand[order], np.full(k - have, cand[order][0] if have else 0)])
        mine = mine[np.lexsort((mine, sq_dists(Q[r], X[mine])))]
        rows[r] = np.concatenate([mine, np.full(k - have, mine[0] if have else 0)])
    assert_same_neighbours_raw(Q, X, rows, full, d)


def assert_same_neighbours_raw(pts, X, got, want, d):
    """The tie rule on lists that may repeat their first row as padding."""
    diff = np.argwhere(got != want)
    for r, c in diff:
        da, db = sq_dists(pts[r], X[got[r, c]][None])[0], sq_dists(pts[r], X[want[r, c]][None])[0]
        assert abs(da - db) <= (2 + 0.5 * np.sqrt(d)) * np.spacing(np.float32(max(da, db))), (r, c, da, db)
    assert len(diff) <= 0.002 * got.size


@functools.lru_cache(maxsize=None)
def kmeans_case(d, k, n):
    """A Gaussian table, 700 queries and scikit-learn's exact neighbours of both kinds of query (computed once)."""
    from sklearn.neighbors import NearestNeighbors

    rng = np.random.default_rng(100 * d + k)
    X = rng.normal(size=(n, d)).astype(np.float32)
    Q = rng.normal(size=(700, d)).astype(np.float32)
    bi = rng.choice(n, size=700, replace=False)
    bi[:3] = [0, n // 2, n - 1]
    ref = NearestNeighbors(n_neighbors=k + 1, algorithm="brute").fit(X)
    want = ref.kneighbors(Q, n_neighbors=k, return_distance=False)
    want_b = ref.kneighbors(X[bi], return_distance=False)[:, 1:]
    for a in (X, Q, bi, want, want_b):
        a.setflags(write=False)
    return X, Q, bi, want, want_b


@pytest.mark.parametrize("d,k,n", [(8, 50, 40000), (40, 30, 25000)])
def test_probing_every_cell_is_the_exact_search(d, k, n):
    from muygpys_amd.neighbors import NN_Wrapper

    X, Q, bi, want, want_b = kmeans_case(d, k, n)
    nn = NN_Wrapper(to_dev(X), k, nn_method="ivf", nlist=64, nprobe=64, kmeans_iters=4)
    got = nn.get_nns(to_dev(Q))[0].cpu().numpy()
    assert int(nn.last_short.sum()) == 0
    assert_same_neighbours(Q, X, got, want, d, "test")
    got_b = nn.get_batch_nns(to_dev(bi))[0].cpu().numpy()
    assert int(nn.last_short.sum()) == 0
    assert_same_neighbours(X[bi], X, got_b, want_b, d, "batch")
    assert not (got_b == bi[:, None]).any()


def test_batch_queries_return_a_duplicate_but_never_themselves():
    """Exact copies of batch rows elsewhere in the table: the copy comes first, at distance 0 -- the row itself never
    (it is excluded by stored position, not by distance: the exact path's contract)."""
    from muygpys_amd.neighbors import NN_Wrapper

    rng = np.random.default_rng(4)
    n, d, k = 6000, 8, 10
    X = rng.normal(size=(n, d)).astype(np.float32)
    bi = rng.choice(n - 100, size=100, replace=False)
    copies = np.arange(n - 100, n)[rng.permutation(100)]
    X[copies[:60]] = X[bi[:60]]  # (60 of the 100 batch rows have a twin)
    nn = NN_Wrapper(to_dev(X), k, nn_method="ivf", nlist=32, nprobe=4)
    idx, dist = nn.get_batch_nns(to_dev(bi))
    idx, dist = idx.cpu().numpy(), dist.cpu().numpy()
    assert not (idx == bi[:, None]).any()
    assert np.array_equal(idx[:60, 0], copies[:60]) and (dist[:60, 0] == 0).all()
    assert (dist[60:, 0] > 0).all() and (dist[:, 1] > 0).all()
    # ... and from the twin's side
    idx2, dist2 = nn.get_batch_nns(to_dev(copies[:60]))
    assert np.array_equal(idx2.cpu().numpy()[:, 0], bi[:60]) and (dist2.cpu().numpy()[:, 0] == 0).all()


def test_short_candidate_sets_are_flagged_and_answered_exactly():
    """Well separated cells of 5, 1, 3, 2 000 and 40 rows, one probe, k = 10: a query next to a small cell has too few
    candidates, the only row of the one-row cell has none at all once it is excluded itself."""
    from muygpys_amd.neighbors import NN_Wrapper

    rng = np.random.default_rng(5)
    d, k = 4, 10
    lengths = [5, 1, 3, 2000, 40]
    centroids = (50.0 * np.eye(5, d, dtype=np.float32) + np.float32(3.0))
    centroids[4] = -50.0
    assignment = np.repeat(np.arange(5), lengths)
    X = (centroids[assignment] + rng.normal(size=(len(assignment), d))).astype(np.float32)
    shuffle = rng.permutation(len(X))
    X, assignment = X[shuffle], assignment[shuffle]
    nn = NN_Wrapper._from_cells(to_dev(X), k, to_dev(centroids), to_dev(assignment), nprobe=1)
    Q = (centroids[np.arange(40) % 5] + rng.normal(size=(40, d))).astype(np.float32)
    want, short = restated_search(nn, Q, X, k)
    assert np.array_equal(short, np.arange(40) % 5 < 3)
    got = nn.get_nns(to_dev(Q))[0].cpu().numpy()
    assert np.array_equal(nn.last_short.cpu().numpy().astype(bool), short)
    assert_same_neighbours(Q, X, got, want, d)
    assert_same_neighbours(Q[short], X, got[short], exact_neighbours(Q[short], X, k), d)
    # batch queries: the lone row of cell 1, a row of cell 0 (4 candidates left), rows of cells 3 and 4 (enough)
    bi = np.array([np.flatnonzero(assignment == c)[0] for c in (1, 0, 3, 4)])
    gb = nn.get_batch_nns(to_dev(bi))[0].cpu().numpy()
    assert nn.last_short.cpu().tolist() == [1, 1, 0, 0]
    assert_same_neighbours(X[bi], X, gb, exact_neighbours(X[bi], X, k, self_rows=bi), d)
    # the kernel's own lists
    bd, bi_raw, flag = raw_scan(nn, X[bi], nn.probe(to_dev(X[bi])), k, self_rows=bi)
    assert flag.tolist() == [1, 1, 0, 0]
    assert (bi_raw[0] == -1).all() and np.isinf(bd[0]).all() and (bd[0] > 0).all()
    assert (bi_raw[1] >= 0).sum() == 4 and (bi_raw[1] == -1).sum() == 6 and np.isinf(bd[1][bi_raw[1] < 0]).all()
    assert (bi_raw[2:] >= 0).all() and np.isfinite(bd[2:]).all()
    self_pos = nn._inv[to_dev(bi)].cpu().numpy()
    assert not (bi_raw == self_pos[:, None]).any()


def kmeans_objective(x, centroids):
    return float(((x[:, None, :] - centroids[None, :, :]) ** 2).sum(-1).min(1).sum())


def test_index_invariants():
    from muygpys_amd.neighbors import NN_Wrapper

    rng = np.random.default_rng(6)
    n, d, nlist, nprobe = 20000, 8, 50, 7  # (more than 256 rows per cell: k-means runs on a sample)
    X = rng.normal(size=(n, d)).astype(np.float32)
    nn = NN_Wrapper(to_dev(X), 10, nn_method="ivf", nlist=nlist, nprobe=nprobe, kmeans_iters=5, seed=11)
    assert (nn.nlist, nn.nprobe) == (nlist, nprobe) and nn.centroids.shape == (nlist, d)
    cs, perm, inv = nn.cell_start.cpu().numpy(), nn._perm.cpu().numpy(), nn._inv.cpu().numpy()
    assert cs.dtype == np.int64 and cs.shape == (nlist + 1,) and cs[0] == 0 and cs[-1] == n and (np.diff(cs) >= 0).all()
    assert np.array_equal(np.sort(perm), np.arange(n)) and np.array_equal(inv[perm], np.arange(n))  # every row in one cell
    stored = nn.train.cpu().numpy()[:, :d].astype(np.float64) + nn._mean.cpu().numpy().astype(np.float64)
    np.testing.assert_allclose(stored, X[perm], rtol=0, atol=2e-6)  # ((x - mean) + mean: two fp32 roundings at |x| < 8)
    # each row's cell is its nearest centroid, near-ties in centroid distance aside
    C = nn.centroids.cpu().numpy().astype(np.float64)
    cd = ((X.astype(np.float64)[:, None, :] - C[None, :, :]) ** 2).sum(-1)
    cell_of = np.empty(n, dtype=np.int64)
    cell_of[perm] = np.repeat(np.arange(nlist), np.diff(cs))
    mine, best = cd[np.arange(n), cell_of], cd.min(1)
    assert (mine <= best * (1 + 1e-5)).all()
    assert (cell_of != cd.argmin(1)).mean() <= 0.01
    # probe(): the nprobe nearest centroids under the same rule
    Q = rng.normal(size=(500, d)).astype(np.float32)
    probes = nn.probe(to_dev(Q)).cpu().numpy()
    assert probes.shape == (500, nprobe) and all(len(set(r.tolist())) == nprobe for r in probes)
    qd = ((Q.astype(np.float64)[:, None, :] - C[None, :, :]) ** 2).sum(-1)
    kth = np.sort(qd, axis=1)[:, nprobe - 1]
    picked = np.take_along_axis(qd, probes, axis=1)
    assert (picked <= kth[:, None] * (1 + 1e-5)).all()
    assert (np.sort(probes, axis=1) != np.sort(np.argsort(qd, axis=1)[:, :nprobe], axis=1)).any(1).mean() <= 0.01
    # Lloyd passes do not raise the objective on the sample they ran on
    sample = nn._kmeans_sample.cpu().numpy()
    assert len(sample) == 256 * nlist and len(set(sample.tolist())) == len(sample)
    xs = nn.train.cpu().numpy().astype(np.float64)[inv[sample]]
    first = nn._kmeans_init.cpu().numpy().astype(np.float64)
    assert len({tuple(r) for r in first}) == nlist  # distinct rows
    assert kmeans_objective(xs, nn._centroids.cpu().numpy().astype(np.float64)) <= kmeans_objective(xs, first)
    # the same seed: the same index, bit for bit; another seed: another index
    again = NN_Wrapper(to_dev(X), 10, nn_method="ivf", nlist=nlist, nprobe=nprobe, kmeans_iters=5, seed=11)
    assert torch.equal(again._centroids, nn._centroids) and torch.equal(again._perm, nn._perm)
    assert torch.equal(again.cell_start, nn.cell_start) and torch.equal(again.train, nn.train)
    other = NN_Wrapper(to_dev(X), 10, nn_method="ivf", nlist=nlist, nprobe=nprobe, kmeans_iters=5, seed=12)
    assert not torch.equal(other._centroids, nn._centroids)


def test_recall_guard():
    """n = 20 000 Gaussian rows at d = 8, k = 10, 8 of 64 cells: the GPU search finds what a numpy restatement of the
    probed search on the same cells finds (they differ by excused ties only), and that is >= 0.90 of the exact
    neighbours -- a numpy simulation of this shape gave 0.974 with 5 Lloyd passes, so only a broken k-means fails."""
    from muygpys_amd.neighbors import NN_Wrapper

    rng = np.random.default_rng(7)
    n, d, k = 20000, 8, 10
    X = rng.normal(size=(n, d)).astype(np.float32)
    Q = rng.normal(size=(400, d)).astype(np.float32)
    nn = NN_Wrapper(to_dev(X), k, nn_method="ivf", nlist=64, nprobe=8)
    got = nn.get_nns(to_dev(Q))[0].cpu().numpy()
    C = nn.centroids.cpu().numpy().astype(np.float64)
    qd = ((Q.astype(np.float64)[:, None, :] - C[None, :, :]) ** 2).sum(-1)
    restated, _ = restated_search(nn, Q, X, k, probes=np.argsort(qd, axis=1)[:, :8])
    exact = exact_neighbours(Q, X, k)

    def recall(found):
        return np.mean([len(set(a.tolist()) & set(b.tolist())) / k for a, b in zip(found, exact)])

    print(f"recall: restated {recall(restated):.4f}, GPU {recall(got):.4f}")
    assert recall(got) >= recall(restated) - 0.005
    assert recall(restated) >= 0.90


@pytest.mark.parametrize("d", [1, 6])
def test_feature_counts_off_the_multiple_of_four(d):
    """Rows are stored zero-padded to the next multiple of 4; at nprobe == nlist the results are the exact path's."""
    from muygpys_amd.neighbors import NN_Wrapper

    rng = np.random.default_rng(8 + d)
    # (d = 1: a table sparse enough for the exact path's own selection -- Gram form, fp32 -- to be exact: the gap between
    # the squared distances of consecutive neighbours grows with the square of the spacing, its rounding does not)
    n, k = (300 if d == 1 else 3000), 7
    X = rng.normal(size=(n, d)).astype(np.float32)
    Q = rng.normal(size=(200, d)).astype(np.float32)
    bi = rng.choice(n, size=200, replace=False)
    Xd = to_dev(X[:, 0] if d == 1 else X)
    nn = NN_Wrapper(Xd, k, nn_method="ivf", nlist=9, nprobe=9)
    exact = NN_Wrapper(Xd, k)
    assert nn.train.shape == (n, 4 if d == 1 else 8) and nn.centroids.shape == (9, d)
    for mine, theirs, pts in ((nn.get_nns(to_dev(Q)), exact.get_nns(to_dev(Q)), Q),
                              (nn.get_batch_nns(to_dev(bi)), exact.get_batch_nns(to_dev(bi)), X[bi])):
        assert_same_neighbours(pts, X, mine[0].cpu().numpy(), theirs[0].cpu().numpy(), d)
        torch.testing.assert_close(mine[1], theirs[1], rtol=1e-5, atol=1e-6)
    assert_same_neighbours(Q, X, nn.get_nns(to_dev(Q))[0].cpu().numpy(), exact_neighbours(Q, X, k), d)


def test_construction_errors_name_the_limit():
    from muygpys_amd.neighbors import NN_Wrapper

    X = torch.randn(500, 8, device="cuda")
    with pytest.raises(ValueError, match="fp32"):
        NN_Wrapper(X.double(), 10, nn_method="ivf")
    with pytest.raises(ValueError, match="d <= 64"):
        NN_Wrapper(torch.randn(500, 65, device="cuda"), 10, nn_method="ivf")
    with pytest.raises(ValueError, match="k <= 64"):
        NN_Wrapper(X, 65, nn_method="ivf")
    with pytest.raises(ValueError, match="nprobe"):
        NN_Wrapper(X, 10, nn_method="ivf", nlist=8, nprobe=9)
    NN_Wrapper(X, 64, nn_method="ivf")  # (the limits themselves are served)
    NN_Wrapper(torch.randn(500, 64, device="cuda"), 10, nn_method="ivf")
