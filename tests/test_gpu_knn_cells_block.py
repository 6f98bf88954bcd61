"""GPU: the block scan of the inverted-cell index (NN_Wrapper.cell_scan = "block", mgp_knn_cells_scan_block) against the
fp64 restatement of the probed search, on the hand-built cells of tests/test_gpu_neighbors_cells.py (0, 1, 63, 64, 65,
0, 129, 1000, 200, 0 rows) and under that file's tie rule: a mismatch only between candidates whose fp64 distances lie
within (2 + sqrt(d) / 2) ulp of fp32, for at most 0.2 % of the entries.  A numpy simulation of the Gram-form fp32
selection (accumulator from -|x|^2/2, one fused step per feature) on this layout, d = 4 .. 64, k = 1 .. 64, mismatched
0 of 1 870 - 19 200 entries against fp64 in every case: the cap excuses nothing the arithmetic needs."""

import numpy as np
import pytest

from tests.test_gpu_neighbors_cells import (assert_same_neighbours, assert_same_neighbours_raw, candidate_rows,
                                            hand_built, restated_search, sq_dists)
from tests.util import to_dev

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("d,k,nprobe", [(4, 1, 1), (4, 1, 3), (8, 50, 10), (8, 64, 3), (20, 30, 5), (40, 50, 3),
                                        (64, 64, 10), (64, 10, 1)])
def test_block_scan_returns_the_k_nearest_of_the_probed_cells(d, k, nprobe):
    """150 test and 150 batch queries (one full block of 128 and one of 22: a wave with few rows), self excluded."""
    nn, X, rng = hand_built(d, nprobe, k)
    nn.cell_scan = "block"
    Q = rng.normal(size=(150, d)).astype(np.float32)
    bi = rng.choice(len(X), size=150, replace=False)
    want, short = restated_search(nn, Q, X, k)
    got = nn.get_nns(to_dev(Q))[0].cpu().numpy()
    assert nn.last_cell_scan == "block" and nn.last_route == "ivf"
    assert np.array_equal(nn.last_short.cpu().numpy().astype(bool), short)
    overflow = nn.last_overflow.cpu().numpy()
    assert overflow.shape == (150,) and set(overflow.tolist()) <= {0, 1}
    if k == 50:  # (some queries' nearest cell is one of the short ones: they start at tau = +inf and overflow)
        assert overflow.any()
    assert_same_neighbours(Q, X, got, want, d, "test")
    want_b, short_b = restated_search(nn, X[bi], X, k, self_rows=bi)
    got_b = nn.get_batch_nns(to_dev(bi))[0].cpu().numpy()
    assert np.array_equal(nn.last_short.cpu().numpy().astype(bool), short_b)
    assert_same_neighbours(X[bi], X, got_b, want_b, d, "batch")
    assert not (got_b == bi[:, None]).any()


def raw_block(nn, q, probes, seed_cell, k):
    """Seed by mgp_knn_cells_scan on one cell per query, then mgp_knn_cells_scan_block: (best_i, overflow, seed full)."""
    from muygpys_amd import _lib

    lib, m = _lib.load(), q.shape[0]
    best_d = torch.empty((m, k), device="cuda")
    best_i = torch.empty((m, k), device="cuda", dtype=torch.int32)
    flag = torch.empty((m,), device="cuda", dtype=torch.int32)
    seed = seed_cell.to(torch.int32)[:, None].contiguous()
    rc = lib.mgp_knn_cells_scan(_lib.ptr(nn.train), nn.train_count, nn._width, _lib.ptr(nn.cell_start), nn.nlist,
                                _lib.ptr(q), m, _lib.ptr(seed), 1, None, k, _lib.ptr(best_d), _lib.ptr(best_i),
                                _lib.ptr(flag), _lib.stream_ptr())
    assert rc == 0
    full = (best_i >= 0).all(1).cpu().numpy()
    sq = torch.cat([(nn.train.double() ** 2).sum(1).float(), torch.full((1,), float("inf"), device="cuda")])
    qn = (q.double() ** 2).sum(1).float()
    skip = seed_cell.to(torch.int64).contiguous()
    overflow = torch.full((m,), -7, device="cuda", dtype=torch.int32)
    rc = lib.mgp_knn_cells_scan_block(_lib.ptr(nn.train), _lib.ptr(sq), nn.train_count, nn._width, _lib.ptr(nn.cell_start),
                                      nn.nlist, _lib.ptr(q), _lib.ptr(qn), m, _lib.ptr(probes), probes.shape[1],
                                      _lib.ptr(skip), None, k, _lib.ptr(best_d), _lib.ptr(best_i), _lib.ptr(overflow),
                                      _lib.stream_ptr())
    assert rc == 0
    torch.cuda.synchronize()
    return best_i.cpu().numpy(), overflow.cpu().numpy(), full


@pytest.mark.parametrize("d,k,nprobe", [(8, 10, 3), (40, 50, 3)])
def test_block_entry_lists_depend_on_the_candidate_set_alone(d, k, nprobe):
    nn, X, rng = hand_built(d, nprobe, k)
    Q = rng.normal(size=(150, d)).astype(np.float32)
    q = nn._pad_features(to_dev(Q, torch.float32) - nn._mean)
    probes, nearest = nn._probe(q)
    probes = probes.sort(1).values.contiguous()
    got, overflow, full = raw_block(nn, q, probes, nearest, k)
    assert set(overflow.tolist()) <= {0, 1} and not overflow[full].any()
    # another query order: every query sits in another block, wave and lane
    shuffle = torch.as_tensor(rng.permutation(150), device="cuda")
    got2, overflow2, _ = raw_block(nn, q[shuffle].contiguous(), probes[shuffle].contiguous(), nearest[shuffle], k)
    back = np.argsort(shuffle.cpu().numpy())
    assert np.array_equal(overflow2[back], overflow)
    keep = overflow == 0
    assert full.any() and (~full).any()  # (both kinds of seed are in the case)
    assert np.array_equal(np.sort(got2[back], axis=1)[keep], np.sort(got, axis=1)[keep])
    # ... and the lists are the fp64 k nearest of the rows of the probed cells
    perm, probes = nn._perm.cpu().numpy(), probes.cpu().numpy()
    rows, want = np.empty((150, k), dtype=np.int64), np.empty((150, k), dtype=np.int64)
    for r in np.flatnonzero(keep):
        cand = candidate_rows(nn, probes[r])
        have = min(k, len(cand))
        assert (got[r] >= 0).sum() == have
        mine = perm[got[r][got[r] >= 0]]
        assert len(set(mine.tolist())) == have and np.isin(mine, cand).all()
        best = cand[np.lexsort((cand, sq_dists(Q[r], X[cand])))[:k]]
        mine = mine[np.lexsort((mine, sq_dists(Q[r], X[mine])))]
        # (short lists padded with their first row on both sides, as tests/test_gpu_neighbors_cells.py does)
        want[r] = np.concatenate([best, np.full(k - have, best[0] if have else 0)])
        rows[r] = np.concatenate([mine, np.full(k - have, mine[0] if have else 0)])
    assert_same_neighbours_raw(Q[keep], X, rows[keep], want[keep], d)


def test_query_scan_stays_the_default_and_other_values_are_refused():
    from muygpys_amd.neighbors import NN_Wrapper

    rng = np.random.default_rng(9)
    X = to_dev(rng.normal(size=(3000, 8)).astype(np.float32))
    Q = to_dev(rng.normal(size=(150, 8)).astype(np.float32))
    nn = NN_Wrapper(X, 10, nn_method="ivf", nlist=12, nprobe=3)  # (the same seed: the same index, bit for bit)
    named = NN_Wrapper(X, 10, nn_method="ivf", nlist=12, nprobe=3, cell_scan="query")
    assert nn.cell_scan == "query" and named.cell_scan == "query"
    idx, dist = nn.get_nns(Q)
    assert nn.last_cell_scan == "query" and nn.last_overflow is None
    idx2, dist2 = named.get_nns(Q)
    assert torch.equal(idx, idx2) and torch.equal(dist, dist2)
    with pytest.raises(ValueError, match="cell_scan"):
        NN_Wrapper(X, 10, nn_method="ivf", cell_scan="nonsense")
    nn.cell_scan = "nonsense"
    with pytest.raises(ValueError, match="cell_scan"):
        nn.get_nns(Q)
