"""GPU: the wide cell scan of the inverted-cell index (mgp_knn_cells_scan_wide, NN_Wrapper.cell_scan = "wide",
1 <= k <= 1024) against the fp64 restatement of the probed search, on the hand-built cells of
tests/test_gpu_neighbors_cells.py (0, 1, 63, 64, 65, 0, 129, 1000, 200, 0 rows) and under that file's tie rule: a
mismatch only between candidates whose fp64 distances lie within (2 + sqrt(d) / 2) ulp of fp32, for at most 0.2 % of the
entries.  A numpy restatement of the kernel's fp32 distance form (four fused partial sums, (s0 + s1) + (s2 + s3)) on
these cases, selected by (distance, position) and compared as sets with the fp64 selection, mismatched 0 entries in
every case, (8, 1024, 10) with its 153 600 entries included: the cap excuses nothing the arithmetic needs."""

import numpy as np
import pytest

from tests.test_gpu_neighbors_cells import (assert_same_neighbours, assert_same_neighbours_raw, candidate_rows,
                                            exact_neighbours, hand_built, raw_scan, restated_search, sq_dists)
from tests.util import to_dev

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


def raw_scan_wide(nn, pts, probes, k, self_rows=None):
    """mgp_knn_cells_scan_wide itself on the index's stored table: (best_d, best_i (stored positions), short_flag)."""
    from muygpys_amd import _lib

    q = nn._pad_features(to_dev(pts, torch.float32) - nn._mean)
    m = q.shape[0]
    probes = probes.to(torch.int32).contiguous()
    self_pos = None if self_rows is None else nn._inv[to_dev(self_rows)].contiguous()
    best_d = torch.full((m, k), -7.0, device="cuda")
    best_i = torch.full((m, k), -7, device="cuda", dtype=torch.int32)
    short = torch.full((m,), -7, device="cuda", dtype=torch.int32)
    rc = _lib.load().mgp_knn_cells_scan_wide(
        _lib.ptr(nn.train), nn.train_count, nn._width, _lib.ptr(nn.cell_start), nn.nlist, _lib.ptr(q), m, _lib.ptr(probes),
        probes.shape[1], _lib.ptr(self_pos), k, _lib.ptr(best_d), _lib.ptr(best_i), _lib.ptr(short), _lib.stream_ptr())
    assert rc == 0
    torch.cuda.synchronize()
    return best_d.cpu().numpy(), best_i.cpu().numpy(), short.cpu().numpy()


def check_raw(nn, X, Q, probes, k, d, self_rows=None):
    """The entry's lists against the fp64 k nearest of the rows of the probed cells, as sets per query; -1 / +inf in
    exactly the slots the candidates cannot fill, and the flag where there are such slots.  Returns the flags."""
    bd, bi, flag = raw_scan_wide(nn, Q, probes, k, self_rows)
    perm, probes = nn._perm.cpu().numpy(), probes.cpu().numpy()
    rows, want = np.empty((len(Q), k), dtype=np.int64), np.empty((len(Q), k), dtype=np.int64)
    for r in range(len(Q)):
        cand = candidate_rows(nn, probes[r], None if self_rows is None else self_rows[r])
        have = min(k, len(cand))
        assert flag[r] == (len(cand) < k), (r, flag[r], len(cand))
        assert (bi[r] >= 0).sum() == have and (bi[r][bi[r] < 0] == -1).all() and np.isposinf(bd[r][bi[r] < 0]).all(), r
        mine = perm[bi[r][bi[r] >= 0]]
        assert len(set(mine.tolist())) == have and np.isin(mine, cand).all(), r
        best = cand[np.lexsort((cand, sq_dists(Q[r], X[cand])))[:k]]
        mine = mine[np.lexsort((mine, sq_dists(Q[r], X[mine])))]
        # (short lists padded with their first row on both sides, as tests/test_gpu_neighbors_cells.py does)
        want[r] = np.concatenate([best, np.full(k - have, best[0] if have else 0)])
        rows[r] = np.concatenate([mine, np.full(k - have, mine[0] if have else 0)])
    assert_same_neighbours_raw(Q, X, rows, want, d)
    return flag


@pytest.mark.parametrize("d,k,nprobe,own", [(4, 65, 10, False), (8, 100, 3, False), (8, 128, 10, False), (8, 129, 10, False),
                                            (40, 256, 10, False), (64, 1000, 10, False), (8, 1024, 10, False),
                                            (8, 1, 1, False), (8, 100, 10, True)])
def test_wide_entry_returns_the_k_nearest_of_its_candidate_set(d, k, nprobe, own):
    nn, X, rng = hand_built(d, nprobe, 1)
    if own:  # batch queries: rows of the table, themselves excluded
        rows = rng.choice(len(X), size=150, replace=False)
        flag = check_raw(nn, X, X[rows], nn.probe(to_dev(X[rows])), k, d, self_rows=rows)
    else:
        Q = rng.normal(size=(150, d)).astype(np.float32)
        flag = check_raw(nn, X, Q, nn.probe(to_dev(Q)), k, d)
    if nprobe == 3:  # (three of these cells often hold fewer than 100 rows)
        assert flag.any() and not flag.all()


@pytest.mark.parametrize("k,own,short", [(129, False, 0), (130, False, 1), (128, True, 0), (129, True, 1)])
def test_fill_edges(k, own, short):
    """The cells of 64 and 65 rows: 129 candidates (128 for a query that is one of them) never reach a selection."""
    nn, X, rng = hand_built(8, 2, 1)
    cs, perm = nn.cell_start.cpu().numpy(), nn._perm.cpu().numpy()
    rows = perm[[cs[3], cs[3] + 63, cs[4], cs[4] + 64]]  # first and last row of either cell
    probes = torch.tensor([[3, 4], [4, 3]] * 2, device="cuda")
    Q = X[rows] if own else rng.normal(size=(4, 8)).astype(np.float32)
    flag = check_raw(nn, X, Q, probes, k, 8, self_rows=rows if own else None)
    assert flag.tolist() == [short] * 4


@pytest.mark.parametrize("d,nprobe", [(8, 10), (64, 3)])
def test_at_k_64_the_lists_are_the_narrow_kernels_bit_for_bit(d, nprobe):
    nn, X, rng = hand_built(d, nprobe, 64)
    Q = rng.normal(size=(150, d)).astype(np.float32)
    probes = nn.probe(to_dev(Q))
    (nd, ni, nf), (wd, wi, wf) = raw_scan(nn, Q, probes, 64), raw_scan_wide(nn, Q, probes, 64)
    assert np.array_equal(nf, wf)
    for dist, pos in ((nd, ni), (wd, wi)):  # each row by (distance bits, position)
        order = np.stack([np.lexsort((p, b)) for p, b in zip(pos, dist.view(np.uint32))])
        dist[:], pos[:] = np.take_along_axis(dist, order, 1), np.take_along_axis(pos, order, 1)
    assert np.array_equal(ni, wi) and np.array_equal(nd.view(np.uint32), wd.view(np.uint32))


@pytest.mark.parametrize("k,nprobe", [(100, 3), (300, 10)])
def test_through_the_wrapper(k, nprobe):
    """Test and batch queries; at nprobe = 3 many queries are short and answered on the dense path."""
    nn, X, rng = hand_built(8, nprobe, 1)
    nn.nn_count = k
    Q = rng.normal(size=(150, 8)).astype(np.float32)
    with pytest.raises(ValueError, match="k <= 64"):  # (the per-query scan, still the default, stops at a wave)
        nn.get_nns(to_dev(Q))
    nn.cell_scan = "wide"
    bi = rng.choice(len(X), size=150, replace=False)
    for pts, own, search in ((Q, None, lambda: nn.get_nns(to_dev(Q))), (X[bi], bi, lambda: nn.get_batch_nns(to_dev(bi)))):
        want, short = restated_search(nn, pts, X, k, self_rows=own)
        idx, dist = search()
        assert (nn.last_cell_scan, nn.last_route, nn.last_overflow) == ("wide", "ivf", None)
        assert np.array_equal(nn.last_short.cpu().numpy().astype(bool), short) and short.any() == (nprobe == 3)
        assert idx.shape == (150, k) and bool((dist[:, 1:] >= dist[:, :-1]).all())
        assert_same_neighbours(pts, X, idx.cpu().numpy(), want, 8)
        assert own is None or not (idx.cpu().numpy() == own[:, None]).any()


def test_probing_every_cell_is_the_exact_search_and_the_limit_is_named():
    from muygpys_amd.neighbors import NN_Wrapper

    rng = np.random.default_rng(11)
    X = rng.normal(size=(20000, 8)).astype(np.float32)
    Q = rng.normal(size=(200, 8)).astype(np.float32)
    nn = NN_Wrapper(to_dev(X), 200, nn_method="ivf", nlist=32, nprobe=32, kmeans_iters=3, cell_scan="wide")
    got = nn.get_nns(to_dev(Q))[0].cpu().numpy()
    assert int(nn.last_short.sum()) == 0 and nn.last_cell_scan == "wide"
    assert_same_neighbours(Q, X, got, exact_neighbours(Q, X, 200), 8)
    for k in (0, 1025):
        with pytest.raises(ValueError, match="k <= 1024"):
            NN_Wrapper(to_dev(X[:2000]), k, nn_method="ivf", cell_scan="wide")
    assert NN_Wrapper(to_dev(X[:2000]), 1024, nn_method="ivf", cell_scan="wide").nn_count == 1024
