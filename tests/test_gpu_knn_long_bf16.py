"""GPU: the split-bf16 pre-filter scan for rows of 68 to 256 features (mgp_knn_scan_long_bf16x3,
csrc/mgp_knn_long_bf16.hip), called directly on the grid of tests/knn_long_cases.py (entry label "bf16": the narrow
entry's sizes, its own seeds) and through NN_Wrapper(scan_kind="prefilter"), against fp64 brute force on the centred data.

The lists hold exact fp32 difference-form distances, so the bound is that of a re-measurement, e = (d + 2) 2^-24 D (one
rounding of the difference, one of the square, d additions of positive terms).  The IN lists are the fp64 k-best of rows
[0, start) re-measured in fp32.  No overflow: whatever the pre-filter can pass beats the query's initial k-th best by less
than SLACK = 4 x 2^-12 x 1.25 |q|max |x|max in distance -- twice, in accumulator units, what margin, error bound (2.4 x
2^-14 x 1.25 at most each) and the raise / lowering of the threshold terms add up to -- so at most 16 such rows (the
queue; one of them the self row, where there is one) may lie in one drain window: 14 at worst on this grid, 11 on the
margin-stress tables, evaluated in fp64 from the inputs alone."""

import types

import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests import knn_long_cases as kc  # noqa: E402
from tests import test_gpu_knn_long as tl  # noqa: E402

U, CAP = kc.U, 16
CASES = [types.SimpleNamespace(**{**vars(c), "entry": "bf16"}) for c in kc.benign_cases("narrow")]


def stress_table(d):
    """Two tight clusters at +-50 e_1, unit noise: |q| |x| ~ 2 600 against distances ~ 2 d, so the pre-filter's absolute
    error (~ 0.4) is of the size of the gaps between neighbours (~ 0.5 around the 30th)."""
    g = torch.Generator().manual_seed(5000 + d)
    n, m = kc.start_of("narrow", 30) + kc.PAST, 129
    X, Q = torch.randn(n, d, generator=g), torch.randn(m, d, generator=g)
    X[:, 0] += 50.0 * (1 - 2 * (torch.arange(n) % 2))
    Q[:, 0] += 50.0 * (1 - 2 * (torch.arange(m) % 2))
    return X, Q


def no_overflow_worst(D, Xc, Qc, k, start, self_idx):
    """The most rows of one drain window the pre-filter can pass, over all queries (inputs only, fp64)."""
    slack = 4 * 2.0**-12 * 1.25 * float((Qc.double() ** 2).sum(1).max().sqrt() * (Xc.double() ** 2).sum(1).max().sqrt())
    shifted = D.clone()
    shifted[:, start:] -= slack
    return kc.worst_window(shifted, k, start) + (0 if self_idx is None else 1)


def run_prefilter(X, Q, k, start, self_idx=None):
    from muygpys_amd import _lib, neighbors as nb

    Xc, Qc = (t.cuda() for t in kc.centre(X, Q))
    self_idx = None if self_idx is None else self_idx.cuda()
    (n, d), m = Xc.shape, Qc.shape[0]
    D = kc.true_distances(Xc, Qc, self_idx)
    sq = (Xc.double() ** 2).sum(1).float()
    sqn = torch.cat([sq, torch.full(((-n) % 64,), float("inf"), device=sq.device)])
    qn = (Qc.double() ** 2).sum(1).float()
    best_i = D[:, :start].topk(k, dim=1, largest=False).indices.to(torch.int32).contiguous()
    diff = Qc[:, None, :] - Xc[best_i.long()]
    best_d = (diff * diff).sum(-1).contiguous()
    kp = nb.packed_width(d)
    c = -0.5 * sq + (nb.prefilter_margin(kp) * 1.25 * float(qn.max().sqrt())) * sq.sqrt()
    c = c + nb.prefilter_raise(kp) * c.abs()
    pX, pQ = nb.NN_Wrapper._pack_bf16(Xc, c, 1.0), nb.NN_Wrapper._pack_bf16(Qc, 1.0, 0.0)
    overflow = torch.zeros((m,), device=Xc.device, dtype=torch.int32)
    ex64 = None if self_idx is None else self_idx.to(torch.int64).contiguous()
    rc = _lib.load().mgp_knn_scan_long_bf16x3(
        _lib.ptr(Xc), _lib.ptr(pX), _lib.ptr(sqn), n, d, _lib.ptr(Qc), _lib.ptr(pQ), _lib.ptr(qn), _lib.ptr(ex64), m, k,
        start, _lib.ptr(best_d), _lib.ptr(best_i), _lib.ptr(overflow), _lib.stream_ptr())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return types.SimpleNamespace(X=Xc, Q=Qc, n=n, d=d, m=m, k=k, start=start, self_idx=self_idx, best_d=best_d,
                                 best_i=best_i, overflow=overflow), D


def check_exact(r, D, label):
    worst = no_overflow_worst(D, r.X, r.Q, r.k, r.start, r.self_idx)
    assert worst <= CAP, f"{worst} rows of one drain window can pass the pre-filter: reseed {label!r}"
    bi = tl.check_lists(r)
    got = D.gather(1, bi)
    nxt = D.topk(r.k + 1, dim=1, largest=False)
    want = nxt.values[:, :r.k]
    rel = (r.d + 2) * U
    own = (r.best_d.double() - got).abs()
    pair = (got.sort(dim=1).values - want).abs()
    assert bool((own <= rel * got).all()), "best_d is not the exact distance of its row"
    assert bool((pair <= rel * want).all()), f"a true neighbour is missing: {int((pair > rel * want).any(1).sum())} of {r.m} queries"
    assert int(r.overflow.sum()) == 0, f"{int(r.overflow.sum())} of {r.m} queries flagged on inputs that cannot overflow"
    clear = (nxt.values[:, r.k] - nxt.values[:, r.k - 1]) > 2 * rel * nxt.values[:, r.k]
    assert int(clear.sum()) > 0
    assert torch.equal(bi[clear].sort(dim=1).values, nxt.indices[clear, :r.k].sort(dim=1).values)


@pytest.mark.parametrize("c", CASES, ids=[kc.case_id(c) for c in CASES])
def test_direct_calls(c):
    X, Q, self_idx = kc.build(c)
    r, D = run_prefilter(X, Q, c.k, c.start, self_idx)
    assert r.n == c.n and r.n % 64 != 0
    check_exact(r, D, kc.case_id(c))


@pytest.mark.parametrize("d", [100, 160, 256])
def test_margin_stress(d):
    X, Q = stress_table(d)
    r, D = run_prefilter(X, Q, 30, kc.start_of("narrow", 30))
    check_exact(r, D, f"stress d={d}")


WRAPPED = [(d, k) for d in (68, 100, 256) for k in (10, 64)]


@pytest.mark.parametrize("d, k", WRAPPED, ids=[f"d{d}-k{k}" for d, k in WRAPPED])
def test_wrapper_takes_the_prefilter(d, k, monkeypatch):
    from muygpys_amd import _lib
    from muygpys_amd.neighbors import NN_Wrapper

    for name in ("MUYGPYS_HIP_KNN_WIDE", "MUYGPYS_HIP_KNN_LONG", "MUYGPYS_HIP_KNN_PAD"):
        monkeypatch.delenv(name, raising=False)
    X, Q, bi = tl.wrapper_problem(d)
    auto, nn = NN_Wrapper(X, k), NN_Wrapper(X, k, scan_kind="prefilter")
    calls, real = [], _lib.load().mgp_knn_scan_long_bf16x3
    monkeypatch.setattr(_lib.load(), "mgp_knn_scan_long_bf16x3", lambda *a: calls.append(1) or real(*a))
    for query, pts, exclude in (("test", nn._pad_features(Q - nn._mean), None), ("batch", nn.train[nn._inv[bi]], bi)):
        (wi, wd), (ai, _) = ((w.get_nns(Q) if exclude is None else w.get_batch_nns(bi)) for w in (nn, auto))
        assert nn.last_route == auto.last_route == "long"
        assert int(nn.last_overflow.sum()) == 0
        D, scale = tl.wrapper_reference(nn, pts, exclude)
        clear = tl.check_wrapper_answer(wi, wd, D, scale, d, k, exclude)
        assert torch.equal(wi[clear], ai[clear])
    assert len(calls) == 2, "mgp_knn_scan_long_bf16x3 served both searches, and only the prefilter object's"


def test_wrapper_at_the_other_shapes():
    from muygpys_amd.neighbors import NN_Wrapper

    X, Q, _ = tl.wrapper_problem(40)
    a, b = NN_Wrapper(X, 10, scan_kind="prefilter"), NN_Wrapper(X, 10, scan_kind="bf16x3")
    assert torch.equal(a.get_nns(Q)[0], b.get_nns(Q)[0]) and a.last_route == "scan"
    X, Q, _ = tl.wrapper_problem(100)
    nn = NN_Wrapper(X, 65, scan_kind="prefilter")
    idx, dist = nn.get_nns(Q)
    assert nn.last_route == "long"
    D, scale = tl.wrapper_reference(nn, nn._pad_features(Q - nn._mean), None)
    tl.check_wrapper_answer(idx, dist, D, scale, 100, 65, None)
    with pytest.raises(ValueError, match="scan_kind"):
        NN_Wrapper(X, 10, scan_kind="bf16")
