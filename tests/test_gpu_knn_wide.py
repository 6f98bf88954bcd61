"""GPU: the exact k-NN scan and finish step for lists of up to 1 024 entries (mgp_knn_scan_wide, mgp_knn_finish_wide:
csrc/mgp_knn_wide.hip), called directly at the shape edges and through NN_Wrapper, against fp64 brute force.

What a direct call is made of (`run_scan`): the table centred on its fp64 mean (queries shifted alike), squared norms
rounded from fp64 and padded with +inf to a multiple of 64, IN lists = the exact k-best over rows [0, start) from torch
(Gram form, fp32), a zero-filled overflow vector.  The result is the entry's unordered lists.

Reference and bound (`check`, the method of tests/test_gpu_knn_scan_edges.py): fp64 distances on the same (centred fp32)
data, self excluded.  Per query the fp64 distances of the returned rows, sorted, are compared element by element with
the sorted true top-k.  A selection that is exact under distances perturbed by at most e returns sorted true distances
within 2 e of the true top-k, with
    e = (d + 5) 2^-24 (|q|^2 + max_x |x|^2)    (Gram form: an fmaf chain of d products from -|x|^2/2, fp32-rounded norms)

No overflow: the wide scan's queue has one slot per column of the 64-row tile and is emptied after every tile, so the
rule under which no query may be flagged is the entry's own contract -- start % 64 == 0 and start >= k (+ 1 with a self
row) -- whatever the inputs are.  `check` asserts that precondition before it looks at the flags.

Query block of the kernel: 128 (four waves of 32 queries)."""

import types
import zlib

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

U = 2.0 ** -24  # unit roundoff of fp32
QB = 128        # queries per workgroup
K_ALL = (1, 63, 64, 65, 127, 128, 129, 1000, 1023, 1024)
D_ALL = (4, 12, 40, 64)
PAST = (1, 63, 64, 64 * 3 + 5)  # rows behind `start`: the last tile is partial, +inf norms do the masking
SELF = ("head", "scanned", None)


def min_start(k):
    """The smallest multiple of 64 that is >= k + 1."""
    return -(-(k + 1) // 64) * 64


def normal(seed_of, n, d, m):
    g = torch.Generator().manual_seed(zlib.crc32(seed_of.encode()))
    return torch.randn(n, d, generator=g).cuda(), torch.randn(m, d, generator=g).cuda()


def self_rows(mode, m, start, n, seed=0):
    """Row each query must not return: inside the head rows, inside the scanned rows, or None."""
    if mode is None:
        return None
    g = torch.Generator().manual_seed(seed)
    lo, hi = (0, start) if mode == "head" else (start, n)
    return (lo + torch.randint(hi - lo, (m,), generator=g)).cuda()


def run_scan(X, Q, k, start, self_idx=None, symbol="mgp_knn_scan_wide"):
    """One direct call; returns the centred data, the unordered lists and the overflow flags."""
    from muygpys_amd import _lib

    mean = X.double().mean(0)
    Xc = (X.double() - mean).float().contiguous()
    Qc = (Q.double() - mean).float().contiguous()
    (n, d), m = Xc.shape, Qc.shape[0]
    sq = (Xc.double() ** 2).sum(1).float()
    sqn = torch.cat([sq, torch.full(((-n) % 64,), float("inf"), device=sq.device)])
    qn = (Qc.double() ** 2).sum(1).float()
    d2 = sq[None, :start] - 2.0 * (Qc @ Xc[:start].T) + qn[:, None]
    if self_idx is not None:
        inside = self_idx < start
        d2[torch.arange(m, device=d2.device)[inside], self_idx[inside]] = float("inf")
    bd, bi = d2.topk(k, dim=1, largest=False)
    best_d, best_i = bd.contiguous(), bi.to(torch.int32).contiguous()
    assert bool(torch.isfinite(best_d).all()), "the IN lists must be finite"
    overflow = torch.zeros((m,), device=Xc.device, dtype=torch.int32)
    ex64 = None if self_idx is None else self_idx.to(torch.int64).contiguous()
    rc = getattr(_lib.load(), symbol)(_lib.ptr(Xc), _lib.ptr(sqn), n, d, _lib.ptr(Qc), _lib.ptr(qn), _lib.ptr(ex64), m, k,
                                      start, _lib.ptr(best_d), _lib.ptr(best_i), _lib.ptr(overflow), _lib.stream_ptr())
    assert rc == 0, (symbol, rc)
    torch.cuda.synchronize()
    return types.SimpleNamespace(X=Xc, Q=Qc, n=n, d=d, m=m, k=k, start=start, self_idx=self_idx, best_d=best_d,
                                 best_i=best_i, overflow=overflow)


def true_distances(r):
    """(m, n) fp64 squared distances of the call's data, +inf at a query's own row."""
    D = torch.cdist(r.Q.double(), r.X.double(), compute_mode="donot_use_mm_for_euclid_dist") ** 2
    if r.self_idx is not None:
        D[torch.arange(r.m, device=D.device), r.self_idx] = float("inf")
    return D


def gram_error(r):
    """e of the module docstring, one per query."""
    return (r.d + 5) * U * ((r.Q.double() ** 2).sum(1) + (r.X.double() ** 2).sum(1).max())


def check_lists(r):
    """Rows in range, pairwise distinct, never self."""
    bi = r.best_i.long()
    assert int(bi.min()) >= 0 and int(bi.max()) < r.n, (int(bi.min()), int(bi.max()), r.n)
    rows = bi.sort(dim=1).values
    assert bool((rows[:, 1:] != rows[:, :-1]).all()), "a row twice in one list"
    if r.self_idx is not None:
        assert not bool((bi == r.self_idx[:, None]).any()), "a query's own row was returned"
    return bi


def check(r, D=None):
    D = true_distances(r) if D is None else D
    bi = check_lists(r)
    got = D.gather(1, bi)
    want = D.topk(r.k, dim=1, largest=False).values  # ascending
    e = gram_error(r)[:, None]
    own = (r.best_d.double() - got).abs()
    pair = (got.sort(dim=1).values - want).abs()
    print(f"\n[wide d={r.d} k={r.k} m={r.m} n={r.n} start={r.start}] 2e {float(2 * e.max()):.3e}, sorted distances off by "
          f"at most {float(pair.max()):.3e}, best_d by {float(own.max()):.3e}, flagged {int(r.overflow.sum())}")
    assert bool((own <= e).all()), f"best_d is not the distance of its row: off by {float((own - e).max()):.3e} past e"
    assert bool((pair <= 2 * e).all()), (
        f"a true neighbour is missing: {int((pair > 2 * e).any(1).sum())} of {r.m} queries, "
        f"worst {float((pair - 2 * e).max()):.3e} past 2e")
    # the rule under which the queues cannot overflow (the entry's contract), then the flags
    assert r.start % 64 == 0 and r.start >= r.k + (0 if r.self_idx is None else 1)
    assert int(r.overflow.sum()) == 0, f"{int(r.overflow.sum())} of {r.m} queries flagged"
    return bi


def direct(name, k, d, m, past, start, self_mode):
    n = start + past
    X, Q = normal(f"{name}/{k}/{d}/{m}/{past}/{start}/{self_mode}", n, d, m)
    return check(run_scan(X, Q, k, start, self_rows(self_mode, m, start, n, seed=k + d)))


# ---- direct calls: every k with every d; the other edges cycle through the cases, then get tests of their own -------
KD = [(k, d) for k in K_ALL for d in D_ALL]


@pytest.mark.parametrize("k, d", KD, ids=[f"k{k}-d{d}" for k, d in KD])
def test_every_k_with_every_d(k, d):
    i = KD.index((k, d))
    m = (1, QB - 1, QB + 1)[i % 3]
    start = (min_start(k), 4096)[(i // 3) % 2]
    direct("kd", k, d, m, PAST[(i // 2) % 4], start, SELF[(i // 4) % 3])


QUERY_EDGES = [(m, k, d) for m in (1, QB - 1, QB + 1) for k, d in ((65, 12), (1024, 40), (129, 64))]


@pytest.mark.parametrize("m, k, d", QUERY_EDGES, ids=[f"m{m}-k{k}-d{d}" for m, k, d in QUERY_EDGES])
def test_query_count_edges(m, k, d):
    direct("m", k, d, m, 64 * 3 + 5, min_start(k), "scanned")


TABLE_EDGES = [(past, big, k) for past in PAST for big in (False, True) for k in (65, 1023)]


@pytest.mark.parametrize("past, big, k", TABLE_EDGES,
                         ids=[f"past{p}-start{'4096' if b else 'min'}-k{k}" for p, b, k in TABLE_EDGES])
def test_table_edges(past, big, k):
    direct("t", k, 40, QB + 1, past, 4096 if big else min_start(k), None)


SELF_EDGES = [(s, k, d) for s in SELF for k, d in ((64, 4), (129, 64), (1024, 12))]


@pytest.mark.parametrize("self_mode, k, d", SELF_EDGES, ids=[f"self-{s}-k{k}-d{d}" for s, k, d in SELF_EDGES])
def test_self_exclusion(self_mode, k, d):
    direct("s", k, d, QB + 1, 64 * 3 + 5, min_start(k), self_mode)


def test_several_blocks_and_a_long_walk():
    """Three workgroups, 40 tiles behind the head rows: start tiles differ, lists are replaced many times over."""
    direct("w", 200, 20, 2 * QB + 3, 40 * 64 - 7, 256, "scanned")


# ---- ties ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k, d", [(101, 8), (1000, 40)])
def test_every_row_twice(k, d):
    """A table in which every row occurs twice (in scattered places): a replace-the-maximum with several entries per
    lane must overwrite ONE entry at the maximum, and must return no row twice."""
    start = min_start(k)
    half = (start + 64 * 6 + 10) // 2
    A, Q = normal(f"ties/{k}/{d}", half, d, QB + 1)
    X = torch.cat([A, A])[torch.randperm(2 * half, generator=torch.Generator().manual_seed(k)).cuda()].contiguous()
    r = run_scan(X, Q, k, start)
    D = true_distances(r)
    check(r, D)
    # (both copies of a row sit at one distance: the sorted distances come in equal pairs, so an odd k cuts a pair --
    # the k-th best is tied with the first row left out -- and an even k ends on one)
    top = D.topk(k + 1, dim=1, largest=False).values
    assert bool((top[:, 0:k - 1:2] == top[:, 1:k:2]).all())
    assert bool((top[:, k] == top[:, k - 1]).all()) == (k % 2 == 1)


# ---- agreement with the narrow scan ----------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 33, 64])
def test_same_sets_as_the_narrow_scan(k):
    d, m, start = 40, 300, 2048  # (2 048 head rows: the narrow scan's own rule for k = 64)
    X, Q = normal(f"narrow/{k}", start + 64 * 5 + 7, d, m)
    wide = run_scan(X, Q, k, start)
    narrow = run_scan(X, Q, k, start, symbol="mgp_knn_scan_f32")
    D = true_distances(wide)
    check(wide, D)
    top = D.topk(k + 1, dim=1, largest=False).values
    clear = ((top[:, k] - top[:, k - 1]) > 4 * gram_error(wide)) & (narrow.overflow == 0)
    assert int(clear.sum()) > m // 2
    a, b = wide.best_i.sort(dim=1).values, narrow.best_i.sort(dim=1).values
    assert torch.equal(a[clear], b[clear])


# ---- the finish step -------------------------------------------------------------------------------------------------
def run_finish(Q, X, cand, row_map, symbol="mgp_knn_finish_wide"):
    from muygpys_amd import _lib

    m, k = cand.shape
    idx = torch.full((m, k), -7, dtype=torch.int64, device=Q.device)
    dist = torch.full((m, k), -7.0, dtype=torch.float32, device=Q.device)
    rc = getattr(_lib.load(), symbol)(_lib.ptr(Q), _lib.ptr(X), X.shape[1], _lib.ptr(cand), m, k, _lib.ptr(row_map),
                                      _lib.ptr(idx), _lib.ptr(dist), _lib.stream_ptr())
    assert rc == 0, (symbol, rc)
    torch.cuda.synchronize()
    return idx, dist


def finish_problem(k, d, m=37, n=3000, nan_row=False):
    """Candidate lists of distinct rows; rows n/2 .. n - 1 are exact copies of rows 0 .. n/2 - 1, so about every list
    holds pairs at exactly equal distances.  ``nan_row``: row 5 has a NaN feature and is in every list."""
    X, Q = normal(f"finish/{k}/{d}", n, d, m)
    X[n // 2:] = X[:n // 2]
    if nan_row:
        X[5, d // 2] = float("nan")
    g = torch.Generator().manual_seed(k)
    cand = torch.stack([torch.randperm(n, generator=g)[:k] for _ in range(m)])
    if nan_row:
        for q in range(m):
            if not bool((cand[q] == 5).any()):
                cand[q, (7 * q) % k] = 5
    return X.contiguous(), Q.contiguous(), cand.to(torch.int32).cuda().contiguous()


@pytest.mark.parametrize("mapped", [False, True], ids=["no-row-map", "row-map"])
@pytest.mark.parametrize("k, d", [(65, 8), (1024, 40), (300, 12)])
def test_finish_orders_and_maps(k, d, mapped):
    X, Q, cand = finish_problem(k, d)
    n, m = X.shape[0], Q.shape[0]
    row_map = torch.randperm(n, generator=torch.Generator().manual_seed(1)).cuda() if mapped else None
    idx, dist = run_finish(Q, X, cand, row_map)
    assert bool((dist[:, 1:] >= dist[:, :-1]).all()), "not ascending"
    # the rows of the list, each once, under the map
    rows = idx if row_map is None else torch.argsort(row_map)[idx]
    assert torch.equal(rows.sort(dim=1).values, cand.long().sort(dim=1).values)
    # distances: fp32 difference form against fp64, (d + 2) 2^-24 relative
    ref = ((Q.double()[:, None, :] - X.double()[rows]) ** 2).sum(-1)
    assert bool(((dist.double() - ref).abs() <= (d + 2) * U * ref).all())
    # stable: among equal distances, the order of the list
    pos = torch.full((m, n), -1, dtype=torch.int64, device=X.device)
    pos.scatter_(1, cand.long(), torch.arange(k, device=X.device).expand(m, k).contiguous())
    p = pos.gather(1, rows)
    tied = dist[:, 1:] == dist[:, :-1]
    assert int(tied.sum()) > 0, "the problem was built to have ties"
    assert bool((p[:, 1:] > p[:, :-1])[tied].all()), "equal distances out of list order"


@pytest.mark.parametrize("k", [65, 1024])
def test_finish_puts_a_nan_row_last(k):
    X, Q, cand = finish_problem(k, 8, nan_row=True)
    idx, dist = run_finish(Q, X, cand, None)
    assert bool((idx != -7).all()) and bool((dist != -7.0).all()), "an output slot was not written"
    assert bool((idx[:, -1] == 5).all()) and bool(torch.isnan(dist[:, -1]).all())
    assert not bool(torch.isnan(dist[:, :-1]).any())
    assert bool((dist[:, 1:-1] >= dist[:, :-2]).all())
    assert torch.equal(idx.sort(dim=1).values, cand.long().sort(dim=1).values)


@pytest.mark.parametrize("mapped", [False, True], ids=["no-row-map", "row-map"])
def test_finish_equals_the_narrow_finish_at_64(mapped):
    X, Q, cand = finish_problem(64, 40, nan_row=True)
    row_map = torch.randperm(X.shape[0], generator=torch.Generator().manual_seed(2)).cuda() if mapped else None
    wi, wd = run_finish(Q, X, cand, row_map)
    ni, nd = run_finish(Q, X, cand, row_map, symbol="mgp_knn_finish_f32")
    assert torch.equal(wi, ni)
    assert torch.equal(wd.view(torch.int32), nd.view(torch.int32))  # (bit for bit, the NaN included)


# ---- through NN_Wrapper ----------------------------------------------------------------------------------------------
_TABLES = {}


def wrapper_problem(n, d):
    """One table, 300 test queries and 300 batch rows per (n, d), shared by the k cases and left unchanged."""
    if (n, d) not in _TABLES:
        g = torch.Generator().manual_seed(n + d)
        X, Q = torch.randn(n, d, generator=g).cuda(), torch.randn(300, d, generator=g).cuda()
        bi = torch.randperm(n, generator=g)[:300]
        bi[:5] = torch.tensor([0, 1, 4095, 4096, n - 1])
        _TABLES[(n, d)] = (X, Q, bi.cuda())
    return _TABLES[(n, d)]


def wrapper_reference(nn, pts_centred, exclude):
    """fp64 distances (m, n) in the caller's row order on the wrapper's own centred fp32 data, self excluded."""
    Xc = nn.train if nn._inv is None else nn.train[nn._inv]
    D = torch.cdist(pts_centred.double(), Xc.double(), compute_mode="donot_use_mm_for_euclid_dist") ** 2
    if exclude is not None:
        D[torch.arange(D.shape[0], device=D.device), exclude] = float("inf")
    return D, (pts_centred.double() ** 2).sum(1) + (Xc.double() ** 2).sum(1).max()


def check_wrapper_answer(idx, dist, D, scale, d, k, exclude):
    assert idx.dtype == torch.int64 and idx.shape == dist.shape == (D.shape[0], k)
    assert bool((dist[:, 1:] >= dist[:, :-1]).all()), "not ascending"
    rows = idx.sort(dim=1).values
    assert bool((rows[:, 1:] != rows[:, :-1]).all()) and int(rows.min()) >= 0 and int(rows.max()) < D.shape[1]
    if exclude is not None:
        assert not bool((idx == exclude[:, None]).any())
    want_d, want_i = D.topk(k, dim=1, largest=False)
    # every distance is the fp32 difference form of ITS row, (d + 2) 2^-24 relative ...
    own = D.gather(1, idx)
    assert bool(((dist.double() - own).abs() <= (d + 2) * U * own).all())
    # ... and the sorted fp64 distances of the returned rows are the true top-k within 2e (the selection's Gram form)
    e = ((d + 5) * U * scale)[:, None]
    assert bool(((own.sort(dim=1).values - want_d).abs() <= 2 * e).all()), "a true neighbour is missing"
    # index for index where the fp64 gap to both neighbouring ranks exceeds 4e
    nxt = D.topk(k + 1, dim=1, largest=False).values
    gap_up = nxt[:, 1:] - nxt[:, :-1]                                            # rank j to rank j + 1
    gap_down = torch.cat([torch.full_like(gap_up[:, :1], float("inf")), gap_up[:, :-1]], dim=1)
    clear = (gap_up > 4 * e) & (gap_down > 4 * e)
    assert int(clear.sum()) > 0
    assert torch.equal(idx[clear], want_i[clear])
    return clear


WRAPPED = [(n, d, k) for n in (9001, 12000) for d in (8, 40) for k in (65, 100, 1023)]


@pytest.mark.parametrize("n, d, k", WRAPPED, ids=[f"n{n}-d{d}-k{k}" for n, d, k in WRAPPED])
def test_wrapper_takes_the_wide_route(n, d, k, monkeypatch):
    from muygpys_amd.neighbors import NN_Wrapper

    X, Q, bi = wrapper_problem(n, d)
    monkeypatch.delenv("MUYGPYS_HIP_KNN_WIDE", raising=False)
    nn = NN_Wrapper(X, k)
    assert nn._perm is not None, "shuffled storage"
    answers = {}
    for route, env in (("wide", None), ("dense", "0")):
        if env is not None:
            monkeypatch.setenv("MUYGPYS_HIP_KNN_WIDE", env)
        answers[route, "test"] = nn.get_nns(Q)
        assert nn.last_route == route
        answers[route, "batch"] = nn.get_batch_nns(bi)
        assert nn.last_route == route
    for query, pts, exclude in (("test", (Q - nn._mean), None), ("batch", nn.train[nn._inv[bi]], bi)):
        D, scale = wrapper_reference(nn, pts, exclude)
        (wi, wd), (di, dd) = answers["wide", query], answers["dense", query]
        clear = check_wrapper_answer(wi, wd, D, scale, d, k, exclude)
        print(f"\n[{query} n={n} d={d} k={k}] ranks held to index equality: {float(clear.double().mean()):.3f}, "
              f"ranks at which the two routes name one row: {float((wi == di).double().mean()):.3f}")
        # the same answer from the dense route: the same rows at every clear rank, and at every rank two selections
        # each within 2e of the true top-k whose distances each carry the difference form's (d + 2) 2^-24
        assert torch.equal(di[clear], wi[clear])
        bound = 2 * (d + 2) * U * dd.double() + 4 * ((d + 5) * U * scale)[:, None]
        assert bool(((wd.double() - dd.double()).abs() <= bound).all())


def test_wrapper_routes_stay_where_they_were(monkeypatch):
    """k <= 64 on the narrow scan, small tables and use_scan=False on the dense path, ivf refuses k > 64."""
    from muygpys_amd.neighbors import NN_Wrapper

    monkeypatch.delenv("MUYGPYS_HIP_KNN_WIDE", raising=False)
    X, Q, _ = wrapper_problem(9001, 8)
    for k, kwargs, route in ((64, {}, "scan"), (65, {}, "wide"), (65, dict(use_scan=False), "dense")):
        nn = NN_Wrapper(X, k, **kwargs)
        assert nn.last_route is None
        nn.get_nns(Q)
        assert nn.last_route == route, (k, kwargs)
    small = NN_Wrapper(X[:8192], 65)
    small.get_nns(Q)
    assert small.last_route == "dense"
    wide64 = NN_Wrapper(X.double(), 65)
    wide64.get_nns(Q.double())
    assert wide64.last_route == "dense"
    with pytest.raises(ValueError):
        NN_Wrapper(X, 65, nn_method="ivf")
    ivf = NN_Wrapper(X, 10, nn_method="ivf")
    ivf.get_nns(Q)
    assert ivf.last_route == "ivf"


def test_adversarial_order_is_still_exact():
    """shuffle=False and a table sorted by decreasing distance from the query cluster: every row beats all rows before
    it, every tile is all candidates.  The answer is exact whatever the flags say (here: none, by construction)."""
    from muygpys_amd.neighbors import NN_Wrapper

    g = torch.Generator().manual_seed(3)
    X = torch.randn(10000, 8, generator=g)
    X = X - X.mean(0)
    X = X[(X ** 2).sum(1).argsort(descending=True)].contiguous().cuda()
    Q = (0.01 * torch.randn(200, 8, generator=g)).cuda()  # near the origin
    for k in (65, 300):
        nn = NN_Wrapper(X, k, shuffle=False)
        assert nn._perm is None
        idx, dist = nn.get_nns(Q)
        assert nn.last_route == "wide"
        D, scale = wrapper_reference(nn, Q - nn._mean, None)
        check_wrapper_answer(idx, dist, D, scale, 8, k, None)


def test_the_two_halves_meet():
    """Neighbours at nn_count = 200 from NN_Wrapper (the wide route) into the posterior with path="auto" (the blocked
    factorisation beyond LDS): mean and variance against the fp64 oracle on the same neighbourhoods, at the suite's
    fp32 tolerance.  Inputs as tests/test_gpu_neighbors.py::test_end_to_end_with_true_neighbours (Gaussian d = 40,
    Matern-3/2 at length scale 5), nugget 1e-2."""
    from muygpys_amd.fused import KernelSpec, posterior_mean_var
    from muygpys_amd.neighbors import NN_Wrapper
    from oracle import muygps_oracle as orc
    from tests.util import RTOL, assert_close, to_dev

    rng = np.random.default_rng(5)
    n, d, k = 9001, 40, 200
    X = rng.normal(size=(n, d)).astype(np.float32).astype(np.float64)
    y = np.sin(X[:, 0]) + 0.1 * rng.normal(size=n)
    bi = np.sort(rng.choice(n, size=64, replace=False))
    Xd, yd, bid = to_dev(X, torch.float32), to_dev(y, torch.float32), to_dev(bi)
    nn = NN_Wrapper(Xd, k)
    ni, _ = nn.get_batch_nns(bid)
    assert nn.last_route == "wide" and ni.shape == (64, k)
    mean, var = posterior_mean_var(KernelSpec("matern15", "l2", 5.0, 1e-2), Xd, Xd, bid, ni, yd, path="auto")
    torch.cuda.synchronize()
    m_ref, v_ref = orc.posterior_mean_var(orc.Spec("matern15", "l2", 5.0, 1e-2), X, X, bi, ni.cpu().numpy(), y)
    assert_close(mean.cpu().numpy().reshape(-1), np.asarray(m_ref).reshape(-1), RTOL["float32"], "mean")
    assert_close(var.cpu().numpy().reshape(-1), np.asarray(v_ref).reshape(-1), RTOL["float32"], "var")
