"""GPU: the exact k-NN scans for rows of 68 to 256 features (mgp_knn_scan_long, mgp_knn_scan_long_wide:
csrc/mgp_knn_long.hip), called directly at the shape edges and through NN_Wrapper -- whose exact route now also pads
rows to a multiple of four features -- against fp64 brute force.

Direct calls: the cases, what a call is made of, the reference, the derived bound 2 e with
e = (d + 5) 2^-24 (|q|^2 + max|x|^2) and the no-overflow precondition of the narrow entry are in
tests/knn_long_cases.py (the method of tests/test_gpu_knn_scan_edges.py and tests/test_gpu_knn_wide.py).  The wide
entry's queues cannot overflow by its contract: start % 64 == 0 and start >= k (+ 1 with a self row).

Through NN_Wrapper: the rule of tests/test_gpu_knn_wide.py::check_wrapper_answer on n = 9 001 rows, 300 test queries
and 300 batch rows."""

import types

import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests import knn_long_cases as kc  # noqa: E402

U = kc.U


def run_scan(entry, X, Q, k, start, self_idx=None):
    """One direct call on CPU tensors; returns the centred data (on the device), the unordered lists and the flags."""
    from muygpys_amd import _lib

    Xc, Qc = (t.cuda() for t in kc.centre(X, Q))
    self_idx = None if self_idx is None else self_idx.cuda()
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
    rc = getattr(_lib.load(), kc.SYMBOL[entry])(_lib.ptr(Xc), _lib.ptr(sqn), n, d, _lib.ptr(Qc), _lib.ptr(qn), _lib.ptr(ex64),
                                                m, k, start, _lib.ptr(best_d), _lib.ptr(best_i), _lib.ptr(overflow),
                                                _lib.stream_ptr())
    assert rc == 0, (kc.SYMBOL[entry], rc)
    torch.cuda.synchronize()
    return types.SimpleNamespace(entry=entry, X=Xc, Q=Qc, n=n, d=d, m=m, k=k, start=start, self_idx=self_idx,
                                 best_d=best_d, best_i=best_i, overflow=overflow)


def check_lists(r):
    """Rows in range, pairwise distinct, never self.  (Holds for flagged queries too.)"""
    bi = r.best_i.long()
    assert int(bi.min()) >= 0 and int(bi.max()) < r.n, (int(bi.min()), int(bi.max()), r.n)
    rows = bi.sort(dim=1).values
    assert bool((rows[:, 1:] != rows[:, :-1]).all()), "a row twice in one list"
    if r.self_idx is not None:
        assert not bool((bi == r.self_idx[:, None]).any()), "a query's own row was returned"
    return bi


def check(r, D=None, label=""):
    D = kc.true_distances(r.X, r.Q, r.self_idx) if D is None else D
    # the rule under which no query may be flagged, from the inputs alone, before the flags are looked at
    if r.entry == "narrow":
        worst = kc.worst_window(D, r.k, r.start)
        assert worst <= kc.QUEUE_ROOM, f"{worst} rows of one drain window beat a query's initial k-th best: reseed {label!r}"
    else:
        assert r.start % 64 == 0 and r.start >= r.k + (0 if r.self_idx is None else 1)
    bi = check_lists(r)
    got = D.gather(1, bi)
    want = D.topk(r.k, dim=1, largest=False).values  # ascending
    e = kc.gram_error(r.X, r.Q)[:, None]
    own = (r.best_d.double() - got).abs()
    pair = (got.sort(dim=1).values - want).abs()
    print(f"\n[{label or r.entry} d={r.d} k={r.k} m={r.m} n={r.n} start={r.start}] 2e {float(2 * e.max()):.3e}, sorted "
          f"distances off by at most {float(pair.max()):.3e}, best_d by {float(own.max()):.3e}, flagged {int(r.overflow.sum())}")
    assert bool((own <= e).all()), f"best_d is not the distance of its row: off by {float((own - e).max()):.3e} past e"
    assert bool((pair <= 2 * e).all()), (
        f"a true neighbour is missing: {int((pair > 2 * e).any(1).sum())} of {r.m} queries, "
        f"worst {float((pair - 2 * e).max()):.3e} past 2e")
    assert int(r.overflow.sum()) == 0, f"{int(r.overflow.sum())} of {r.m} queries flagged on inputs that cannot overflow"
    return bi


CASES = kc.benign_cases("narrow") + kc.benign_cases("wide")


@pytest.mark.parametrize("c", CASES, ids=[kc.case_id(c) for c in CASES])
def test_direct_calls(c):
    X, Q, self_idx = kc.build(c)
    r = run_scan(c.entry, X, Q, c.k, c.start, self_idx)
    assert r.n == c.n and r.n % 64 != 0
    bi = check(r, label=kc.case_id(c))
    if c.table != "normal":
        # these tables have no slack: the rows are the true top-k wherever the k-th gap is clear of 4e
        D = kc.true_distances(r.X, r.Q, r.self_idx)
        nxt = D.topk(c.k + 1, dim=1, largest=False)
        e = kc.gram_error(r.X, r.Q)
        clear = (nxt.values[:, c.k] - nxt.values[:, c.k - 1]) > 4 * e
        assert int(clear.sum()) > 0
        assert torch.equal(bi[clear].sort(dim=1).values, nxt.indices[clear, :c.k].sort(dim=1).values)


def adversarial(d, m):
    """All queries at the origin (once centred), the table sorted farthest first: every row beats every earlier one."""
    g = torch.Generator().manual_seed(d)
    X = torch.randn(64 * 9, d, generator=g)
    X = (X.double() - X.double().mean(0)).float()
    X = X[(X.double() ** 2).sum(1).argsort(descending=True)].contiguous()
    Q = X.double().mean(0).float().expand(m, d).contiguous()
    return X, Q


@pytest.mark.parametrize("d", [68, 256])
def test_adversarial_order_flags_every_query_of_the_narrow_entry(d):
    """Each drain meets a whole tile of candidates in a 16-entry queue: every query is flagged, by construction; the
    flagged lists are incomplete by contract, but hold distinct rows of the table."""
    k, m, start = 10, 200, 320
    X, Q = adversarial(d, m)
    r = run_scan("narrow", X, Q, k, start)
    D = kc.true_distances(r.X, r.Q)
    tau0 = D[:, :start].topk(k, dim=1, largest=False).values[:, -1]
    per_tile = (D[:, start:] < tau0[:, None]).reshape(m, 4, 64).sum(-1)
    assert int(per_tile.min()) >= 63 > 16
    check_lists(r)
    assert bool((r.overflow == 1).all()), f"{int((r.overflow == 0).sum())} of {m} queries not flagged"


@pytest.mark.parametrize("d", [68, 256])
def test_adversarial_order_is_exact_on_the_wide_entry(d):
    """The same table: one queue slot per tile column, nothing flagged, the lists exact."""
    X, Q = adversarial(d, 200)
    for k in (10, 65):
        r = run_scan("wide", X, Q, k, 320)
        check(r, label=f"adversarial k={k}")


@pytest.mark.parametrize("entry, k", [("mgp_knn_finish_f32", 64), ("mgp_knn_finish_wide", 1024)])
def test_finish_entries_at_256_features(entry, k):
    """The finish steps have no upper limit on d: fp32 difference-form distances of the candidates against an fp64
    re-measurement, ascending, ties by position in the list, row numbers through row_map."""
    from muygpys_amd import _lib

    d, n, m = 256, 1500, 70
    g = torch.Generator().manual_seed(k)
    X, Q = torch.randn(n, d, generator=g).cuda(), torch.randn(m, d, generator=g).cuda()
    X[7] = X[3]  # (two rows at one distance from every query)
    cand = torch.stack([torch.randperm(n, generator=g)[:k] for _ in range(m)])
    cand[:, 5], cand[:, 2] = 7, 3  # row 7 stands BEHIND row 3 in every list
    fix = (cand == 3) | (cand == 7)
    fix[:, 5] = fix[:, 2] = False
    cand[fix] = 11  # (no third copy of either; row 11 may repeat: the finish step ranks positions, not rows)
    cand = cand.to(torch.int32).cuda().contiguous()
    row_map = torch.randperm(n, generator=g).cuda()
    idx = torch.full((m, k), -1, dtype=torch.int64, device="cuda")
    dist = torch.full((m, k), -1.0, device="cuda")
    rc = getattr(_lib.load(), entry)(_lib.ptr(Q), _lib.ptr(X), d, _lib.ptr(cand), m, k, _lib.ptr(row_map), _lib.ptr(idx),
                                     _lib.ptr(dist), _lib.stream_ptr())
    assert rc == 0
    torch.cuda.synchronize()
    D = torch.cdist(Q.double(), X.double(), compute_mode="donot_use_mm_for_euclid_dist") ** 2
    own = D.gather(1, cand.long())
    assert bool((dist[:, 1:] >= dist[:, :-1]).all()), "not ascending"
    # every output slot written, each the difference form of a candidate: (d + 2) 2^-24 relative
    inv = torch.empty_like(row_map)
    inv[row_map] = torch.arange(n, device="cuda")
    rows = inv[idx]
    assert torch.equal(rows.sort(dim=1).values, cand.long().sort(dim=1).values), "row_map applied to the candidates"
    assert bool(((dist.double() - D.gather(1, rows)).abs() <= (d + 2) * U * D.gather(1, rows)).all())
    # the order is that of the fp64 distances wherever those are (d + 2) 2^-23 apart
    order = own.argsort(dim=1, stable=True)
    sorted_own = own.gather(1, order)
    clear = torch.ones_like(sorted_own, dtype=torch.bool)
    gap = (sorted_own[:, 1:] - sorted_own[:, :-1]) > 2 * (d + 2) * U * sorted_own[:, 1:]
    clear[:, 1:] &= gap
    clear[:, :-1] &= gap
    assert torch.equal(rows[clear], cand.long().gather(1, order)[clear])
    # the tie: rows 3 and 7 are bit-equal, the earlier list position comes first
    at3, at7 = (rows == 3).nonzero()[:, 1], (rows == 7).nonzero()[:, 1]
    assert at3.numel() == at7.numel() == m and bool((at7 == at3 + 1).all())


# ---- through NN_Wrapper ------------------------------------------------------------------------------------------------
N_WRAP = 9001
_TABLES = {}


def wrapper_problem(d):
    """One table, 300 test queries and 300 batch rows per d, shared by the k cases and left unchanged."""
    if d not in _TABLES:
        g = torch.Generator().manual_seed(N_WRAP + d)
        X, Q = torch.randn(N_WRAP, d, generator=g).cuda(), torch.randn(300, d, generator=g).cuda()
        bi = torch.randperm(N_WRAP, generator=g)[:300]
        bi[:5] = torch.tensor([0, 1, 4095, 4096, N_WRAP - 1])
        _TABLES[d] = (X, Q, bi.cuda())
    return _TABLES[d]


def wrapper_reference(nn, pts_stored, exclude):
    """fp64 distances (m, n) in the caller's row order on the wrapper's own centred (and padded) fp32 data."""
    Xc = nn.train if nn._inv is None else nn.train[nn._inv]
    D = torch.cdist(pts_stored.double(), Xc.double(), compute_mode="donot_use_mm_for_euclid_dist") ** 2
    if exclude is not None:
        D[torch.arange(D.shape[0], device=D.device), exclude] = float("inf")
    return D, (pts_stored.double() ** 2).sum(1) + (Xc.double() ** 2).sum(1).max()


def check_wrapper_answer(idx, dist, D, scale, d, k, exclude):
    """tests/test_gpu_knn_wide.py::check_wrapper_answer, with d the STORED width (the length of the fmaf chains)."""
    assert idx.dtype == torch.int64 and idx.shape == dist.shape == (D.shape[0], k)
    assert bool((dist[:, 1:] >= dist[:, :-1]).all()), "not ascending"
    rows = idx.sort(dim=1).values
    assert bool((rows[:, 1:] != rows[:, :-1]).all()) and int(rows.min()) >= 0 and int(rows.max()) < D.shape[1]
    if exclude is not None:
        assert not bool((idx == exclude[:, None]).any())
    want_d, want_i = D.topk(k, dim=1, largest=False)
    own = D.gather(1, idx)
    assert bool(((dist.double() - own).abs() <= (d + 2) * U * own).all())
    e = ((d + 5) * U * scale)[:, None]
    assert bool(((own.sort(dim=1).values - want_d).abs() <= 2 * e).all()), "a true neighbour is missing"
    nxt = D.topk(k + 1, dim=1, largest=False).values
    gap_up = nxt[:, 1:] - nxt[:, :-1]
    gap_down = torch.cat([torch.full_like(gap_up[:, :1], float("inf")), gap_up[:, :-1]], dim=1)
    clear = (gap_up > 4 * e) & (gap_down > 4 * e)
    assert int(clear.sum()) > 0
    assert torch.equal(idx[clear], want_i[clear])
    return clear


PADDED, LONG = (1, 2, 3, 10, 30), (68, 100, 256)
WRAPPED = [(d, k) for d in PADDED + LONG for k in (10, 65)]
SWITCH = {True: "MUYGPYS_HIP_KNN_LONG", False: "MUYGPYS_HIP_KNN_PAD"}


@pytest.mark.parametrize("d, k", WRAPPED, ids=[f"d{d}-k{k}" for d, k in WRAPPED])
def test_wrapper_routes_and_answers(d, k, monkeypatch):
    from muygpys_amd.neighbors import NN_Wrapper

    for name in ("MUYGPYS_HIP_KNN_WIDE", "MUYGPYS_HIP_KNN_LONG", "MUYGPYS_HIP_KNN_PAD"):
        monkeypatch.delenv(name, raising=False)
    X, Q, bi = wrapper_problem(d)
    table = X[:, 0].contiguous() if d == 1 else X  # (a 1-D tensor input (n,) still works)
    nn = NN_Wrapper(table, k)
    width = max(4, -(-d // 4) * 4)
    assert nn.feature_count == d and nn.train_count == N_WRAP and nn.train.shape == (N_WRAP, width)
    assert nn._perm is not None, "shuffled storage"
    new_route = "long" if d > 64 else ("wide" if k > 64 else "scan")
    switch = SWITCH[d > 64]
    answers = {}
    for route, env in ((new_route, None), ("dense", "0")):
        if env is not None:
            monkeypatch.setenv(switch, env)
        answers[route, "test"] = nn.get_nns(Q[:, 0] if d == 1 else Q)
        assert nn.last_route == route, (nn.last_route, route)
        answers[route, "batch"] = nn.get_batch_nns(bi)
        assert nn.last_route == route, (nn.last_route, route)
    for query, pts, exclude in (("test", nn._pad_features(Q - nn._mean), None), ("batch", nn.train[nn._inv[bi]], bi)):
        D, scale = wrapper_reference(nn, pts, exclude)
        (wi, wd), (di, dd) = answers[new_route, query], answers["dense", query]
        clear = check_wrapper_answer(wi, wd, D, scale, width, k, exclude)  # (self excluded, the caller's row numbers)
        print(f"\n[{query} d={d} k={k} {new_route}] ranks held to index equality: {float(clear.double().mean()):.3f}, "
              f"ranks at which the two routes name one row: {float((wi == di).double().mean()):.3f}")
        # the same answer from the dense route (the rule of test_wrapper_takes_the_wide_route)
        assert torch.equal(di[clear], wi[clear])
        bound = 2 * (width + 2) * U * dd.double() + 4 * ((width + 5) * U * scale)[:, None]
        assert bool(((wd.double() - dd.double()).abs() <= bound).all())


def test_rows_wider_than_256_stay_dense():
    from muygpys_amd.neighbors import NN_Wrapper

    g = torch.Generator().manual_seed(260)
    X, Q = torch.randn(N_WRAP, 260, generator=g).cuda(), torch.randn(50, 260, generator=g).cuda()
    nn = NN_Wrapper(X, 10)
    assert nn._perm is None and nn.train.shape == (N_WRAP, 260)
    idx, dist = nn.get_nns(Q)
    assert nn.last_route == "dense"
    D, scale = wrapper_reference(nn, Q - nn._mean, None)
    check_wrapper_answer(idx, dist, D, scale, 260, 10, None)
