"""GPU: the long-row cell scan of the inverted-cell index (mgp_knn_cells_scan_long, NN_Wrapper.cell_scan = "long",
65 <= d <= 256, 1 <= k <= 1024) against fp64 brute force over the rows of the probed cells, on hand-built cells of
0, 1, 64, 65, 700, 130, 0 and 1040 rows.  Compared by distances: the fp64 distances of the returned rows, sorted, against
the reference's k smallest at rtol = 1e-5 (fp32 near-ties may swap equals), the rows distinct, inside the probed cells
and never the excluded one; the returned distances at the bound of tests/test_gpu_neighbors_cells.py."""

import numpy as np
import pytest

from tests.util import to_dev

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

CELL_LENGTHS = (0, 1, 64, 65, 700, 130, 0, 1040)


def build(X, k, nprobe, centroids=None, deal=True):
    """An index over cells of CELL_LENGTHS rows: dealt at random, or (deal=False) the table's rows in order."""
    from muygpys_amd.neighbors import NN_Wrapper

    rng = np.random.default_rng(0)
    assignment = np.repeat(np.arange(len(CELL_LENGTHS)), CELL_LENGTHS)
    if centroids is None:
        centroids = rng.normal(size=(len(CELL_LENGTHS), X.shape[1])).astype(np.float32)
    return NN_Wrapper._from_cells(to_dev(X), k, to_dev(centroids), to_dev(rng.permutation(assignment) if deal else assignment),
                                  nprobe=nprobe, cell_scan="long")


def check_against_brute_force(nn, X, pts, idx, dist, k, own=None):
    """fp64 brute force over the rows of the cells nn.probe names (over the table for a query they leave short)."""
    assert (nn.last_cell_scan, nn.last_route) == ("long", "ivf")
    idx, dist, short = idx.cpu().numpy(), dist.cpu().numpy(), nn.last_short.cpu().numpy()
    probes = nn.probe(to_dev(pts)).cpu().numpy()
    cs, perm = nn.cell_start.cpu().numpy(), nn._perm.cpu().numpy()
    X64, P64 = X.astype(np.float64), pts.astype(np.float64)
    assert idx.shape == dist.shape == (len(pts), k)
    for r in range(len(pts)):
        cand = np.concatenate([perm[cs[c]:cs[c + 1]] for c in probes[r]])
        cand = cand if own is None else cand[cand != own[r]]
        assert short[r] == (len(cand) < k), r
        if short[r]:
            cand = np.setdiff1d(np.arange(len(X)), [] if own is None else [own[r]])
        want = np.sort(((X64[cand] - P64[r]) ** 2).sum(1))[:k]
        assert len(set(idx[r].tolist())) == k and np.isin(idx[r], cand).all(), r
        mine = ((X64[idx[r]] - P64[r]) ** 2).sum(1)
        np.testing.assert_allclose(np.sort(mine), want, rtol=1e-5, err_msg=str(r))
        np.testing.assert_allclose(dist[r], mine, rtol=1e-5, atol=1e-6, err_msg=str(r))
    return short


@pytest.mark.parametrize("k,nprobe", [(1, 1), (10, 3), (64, 8), (65, 3), (200, 8), (200, 1)])
@pytest.mark.parametrize("d", [65, 68, 100, 128, 252, 256])
def test_long_scan_returns_the_k_nearest_of_its_candidate_set(d, k, nprobe):
    """Padded, smallest, with a tail chunk, whole chunks only, widest; both lists; one cell, some, every cell (= the exact
    search).  One or three of these cells often hold fewer than k rows: those queries are answered exactly."""
    rng = np.random.default_rng(1000 * d + k)
    X = rng.normal(size=(sum(CELL_LENGTHS), d)).astype(np.float32)
    Q = rng.normal(size=(96, d)).astype(np.float32)
    nn = build(X, k, nprobe)
    short = check_against_brute_force(nn, X, Q, *nn.get_nns(to_dev(Q)), k)
    assert nprobe < len(CELL_LENGTHS) or not short.any()  # (every cell: brute force over the whole table)


@pytest.mark.parametrize("case", ["equal_head", "far_half", "tie_at_tau"])
@pytest.mark.parametrize("d,k", [(100, 10), (256, 65)])
def test_pruning_edges(case, d, k):
    rng = np.random.default_rng(7)
    X = rng.normal(size=(sum(CELL_LENGTHS), d)).astype(np.float32)
    Q = rng.normal(size=(64, d)).astype(np.float32)
    if case == "equal_head":  # nothing separates the rows before the last chunks
        X[:, :64] = X[0, :64]
    elif case == "far_half":  # every other row leaves at the first chunk
        X[::2, 0] += 100.0
    else:  # the k-th nearest row of query 0, once more in the last cell (the table's last rows, deal=False)
        X[-1] = X[np.argsort(((X.astype(np.float64) - Q[0]) ** 2).sum(1))[k - 1]]
    nn = build(X, k, len(CELL_LENGTHS), deal=False)
    check_against_brute_force(nn, X, Q, *nn.get_nns(to_dev(Q)), k)


@pytest.mark.parametrize("d,k,nprobe", [(100, 10, 3), (68, 200, 8)])
def test_batch_queries_never_return_themselves(d, k, nprobe):
    rng = np.random.default_rng(d)
    X = rng.normal(size=(sum(CELL_LENGTHS), d)).astype(np.float32)
    rows = rng.choice(len(X), size=96, replace=False)
    nn = build(X, k, nprobe)
    idx, dist = nn.get_batch_nns(to_dev(rows))
    assert not (idx.cpu().numpy() == rows[:, None]).any()
    check_against_brute_force(nn, X, X[rows], idx, dist, k, own=rows)


def test_short_queries_are_flagged_and_answered_exactly():
    """One probe, k = 70: only the cells of 700, 130 and 1040 rows fill a list."""
    rng = np.random.default_rng(3)
    X = rng.normal(size=(sum(CELL_LENGTHS), 100)).astype(np.float32)
    Q = rng.normal(size=(64, 100)).astype(np.float32)
    centroids = np.zeros((8, 100), dtype=np.float32)
    centroids[:, 0] = 10 * np.arange(8)
    Q[:, 0] += 10 * (np.arange(64) % 8)  # query r probes cell r % 8
    nn = build(X, 70, 1, centroids=centroids)
    short = check_against_brute_force(nn, X, Q, *nn.get_nns(to_dev(Q)), 70)
    assert np.array_equal(short != 0, np.isin(np.arange(64) % 8, (0, 1, 2, 3, 6)))


def test_construction_and_attribute_errors_name_the_limit():
    from muygpys_amd.neighbors import NN_Wrapper

    rng = np.random.default_rng(9)  # (a generator of its own: no test here draws from a global one)
    for d in (64, 257):
        with pytest.raises(ValueError, match="65 <= d <= 256"):
            NN_Wrapper(to_dev(rng.normal(size=(500, d)).astype(np.float32)), 10, nn_method="ivf", cell_scan="long")
    X = to_dev(rng.normal(size=(2000, 100)).astype(np.float32))
    with pytest.raises(ValueError, match="d <= 64"):
        NN_Wrapper(X, 10, nn_method="ivf", cell_scan="query")
    with pytest.raises(ValueError, match="fp32 only"):
        NN_Wrapper(X.double(), 10, nn_method="ivf", cell_scan="long")
    with pytest.raises(ValueError, match="k <= 1024"):
        NN_Wrapper(X, 1025, nn_method="ivf", cell_scan="long")
    nn = NN_Wrapper(X, 10, nn_method="ivf", cell_scan="long", kmeans_iters=2)
    nn.cell_scan = "query"  # (a plain attribute, read at every search)
    with pytest.raises(ValueError, match="d <= 64"):
        nn.get_nns(X[:5])
    short = NN_Wrapper(X[:, :40].contiguous(), 10, nn_method="ivf", kmeans_iters=2)
    short.cell_scan = "long"
    with pytest.raises(ValueError, match="65 <= d <= 256"):
        short.get_nns(X[:5, :40])


@pytest.mark.parametrize("d,k", [(100, 30), (252, 100)])
def test_a_query_gets_the_same_rows_alone_in_a_batch_and_in_the_reversed_batch(d, k):
    rng = np.random.default_rng(5)
    X = rng.normal(size=(sum(CELL_LENGTHS), d)).astype(np.float32)
    Q = to_dev(rng.normal(size=(70, d)).astype(np.float32))
    nn = build(X, k, 3)
    batch, flipped = nn.get_nns(Q)[0], nn.get_nns(Q.flip(0))[0].flip(0)
    assert torch.equal(batch, flipped)
    for r in (0, 33, 69):
        assert torch.equal(nn.get_nns(Q[r:r + 1])[0][0], batch[r])
