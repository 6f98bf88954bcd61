"""GPU: the split-bf16 pre-filter scan of the wide lists (mgp_knn_scan_wide_bf16x3, csrc/mgp_knn_wide_bf16.hip), called
directly and through NN_Wrapper(scan_kind="prefilter"), against fp64 brute force on the centred data.

The lists hold fp32 difference-form re-measurements, so the bound is e = (d + 2) 2^-24 D (one rounding of the difference,
one of the square, d additions of positive terms): every best_d within e of its row's fp64 distance, the sorted list
within e of the true top-k, the index sets equal wherever the fp64 gap at rank k exceeds 2 e.  The IN lists are the fp64
k-best of rows [0, start) re-measured in fp32.  The queue is a ring of bit masks and cannot overflow: no precondition.

The drain interval is clamp(rows seen / 64, one tile, W tiles) rows, W = mgp_knn_wide_bf16_window(): behind `start` =
4 096 w head rows a window holds w tiles, so the window cases start from 4 096 W rows (and one from 3 x 4 096)."""

import types

import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests import test_gpu_knn_long_bf16 as tb  # noqa: E402
from tests import test_gpu_knn_wide as tw  # noqa: E402

kc, U = tb.kc, tw.U


def run(X, Q, k, start, self_idx=None, cut=None):
    from muygpys_amd import _lib
    from muygpys_amd.neighbors import NN_Wrapper

    cut = k if cut is None else cut
    Xc, Qc = (t.cuda() for t in kc.centre(X, Q))
    (n, d), m = Xc.shape, Qc.shape[0]
    # (256 queries at a time: past 2^24 pairs in one call torch.cdist's exact mode returned zeros on the ROCm build at hand)
    D = torch.cat([kc.true_distances(Xc, Qc[s:s + 256], None if self_idx is None else self_idx[s:s + 256])
                   for s in range(0, m, 256)])
    sq =(Xc.double() ** 2).sum(1).float()
    sqn = torch.cat([sq, torch.full(((-n) % 64,), float("inf"), device=sq.device)])
    qn = (Qc.double() ** 2).sum(1).float()
    best_i = D[:, :start].topk(k, dim=1, largest=False).indices.to(torch.int32).contiguous()
    diff = Qc[:, None, :] - Xc[best_i.long()]
    best_d = (diff * diff).sum(-1).contiguous()
    c = -0.5 * sq + (2.0**-14 * 1.25 * float(qn.max().sqrt())) * sq.sqrt()
    c = c + 2.0**-15 * c.abs()
    pX, pQ = NN_Wrapper._pack_bf16(Xc, c, 1.0), NN_Wrapper._pack_bf16(Qc, 1.0, 0.0)
    overflow = torch.zeros((m,), device=Xc.device, dtype=torch.int32)
    ex64 = None if self_idx is None else self_idx.to(torch.int64).contiguous()
    rc = _lib.load().mgp_knn_scan_wide_bf16x3(
        _lib.ptr(Xc), _lib.ptr(pX), _lib.ptr(sqn), n, d, _lib.ptr(Qc), _lib.ptr(pQ), _lib.ptr(qn), _lib.ptr(ex64), m, k,
        start, _lib.ptr(best_d), _lib.ptr(best_i), _lib.ptr(overflow), _lib.stream_ptr())
    assert rc == 0, rc
    torch.cuda.synchronize()
    r = types.SimpleNamespace(X=Xc, Q=Qc, n=n, d=d, m=m, k=k, start=start, self_idx=self_idx, best_d=best_d,
                              best_i=best_i, overflow=overflow)
    bi = tw.check_lists(r)
    got, nxt, rel = D.gather(1, bi), D.topk(k + 1, dim=1, largest=False), (d + 2) * U
    want = nxt.values[:, :k]
    own, pair = (best_d.double() - got).abs(), (got.sort(dim=1).values - want).abs()
    print(f"\n[d={d} k={k} m={m} n={n} start={start}] best_d off by {float((own / got).max()):.2e} of e/D = {rel:.2e}, "
          f"sorted lists by {float((pair / want).max()):.2e}")
    assert bool((own <= rel * got).all()), "best_d is not the exact distance of its row"
    assert bool((pair <= rel * want).all()), f"a true neighbour is missing: {int((pair > rel * want).any(1).sum())} of {m} queries"
    assert int(overflow.sum()) == 0, "the overflow flags are never written"
    # (`cut` < k where the table ties the k-th best with the first row left out: the first `cut` ranks are held then)
    clear = (nxt.values[:, cut] - nxt.values[:, cut - 1]) > 2 * rel * nxt.values[:, cut]
    assert int(clear.sum()) > 0
    assert bool((nxt.indices[clear, :cut, None] == bi[clear][:, None, :]).any(2).all()), "a clear neighbour is not in the list"


def direct(name, d, k, m, start, past, self_mode=None):
    X, Q = tw.normal(f"bf16/{name}/{d}/{k}/{m}/{start}/{past}/{self_mode}", start + past, d, m)
    run(X, Q, k, start, tw.self_rows(self_mode, m, start, start + past, seed=k + d))


KD = [(d, k) for d in (4, 28, 44, 60, 64) for k in (65, 128, 129, 1024)]


@pytest.mark.parametrize("d, k", KD, ids=[f"d{d}-k{k}" for d, k in KD])
def test_every_packed_width_with_every_list_shape(d, k):
    direct("kd", d, k, 129, k, 64 * 3 + 5)


WALKS = {"1": lambda W: 1, "W-1": lambda W: W - 1, "W": lambda W: W, "W+1": lambda W: W + 1, "2W+1": lambda W: 2 * W + 1}


@pytest.mark.parametrize("last", [1, 63])
@pytest.mark.parametrize("walk", sorted(WALKS))
def test_window_edges(walk, last):
    from muygpys_amd import _lib

    W = _lib.load().mgp_knn_wide_bf16_window()
    direct("w", 12, 65, 129, 4096 * W, 64 * (WALKS[walk](W) - 1) + last)


@pytest.mark.parametrize("m, heads", [(257, None), (513, None), (129, 3)], ids=["m257", "m513", "three-tile-windows"])
def test_several_workgroups_wrap_inside_a_window(m, heads):
    from muygpys_amd import _lib

    W = _lib.load().mgp_knn_wide_bf16_window()
    direct("g", 40, 100, m, 4096 * (heads or W), 64 * 2 * W + 5, "scanned")


@pytest.mark.parametrize("self_mode", tw.SELF, ids=[str(s) for s in tw.SELF])
def test_self_rows(self_mode):
    direct("s", 28, 129, 129, 130, 64 * 3 + 5, self_mode)


@pytest.mark.parametrize("k, start", [(65, 4096 * 8), (1023, 1023)])
def test_farthest_first_table(k, start):
    """Rows in order of decreasing distance from the queries' cluster: every scanned row beats tau, every mask fills."""
    X, _ = tw.normal(f"far/{k}", start + 64 * 9 + 3, 8, 1)
    X = (X - X.mean(0))
    X = X[(X ** 2).sum(1).argsort(descending=True)].contiguous()
    run(X, 0.01 * tw.normal(f"far-q/{k}", 1, 8, 129)[1], k, start)


def test_every_row_twice():
    """Ties at tau: no row twice (check_lists).  Both copies of a row sit at one distance, so the odd k cuts a pair and
    the k-th best is tied with the first row left out: the index sets are held to the first k - 1 ranks."""
    k, d = 101, 8
    half = (k + 64 * 6 + 10) // 2
    A, Q = tw.normal(f"bf16-ties/{k}/{d}", half, d, 129)
    X = torch.cat([A, A])[torch.randperm(2 * half, generator=torch.Generator().manual_seed(k)).cuda()].contiguous()
    run(X, Q, k, k, cut=k - 1)


@pytest.mark.parametrize("d", [40, 64])
def test_margin_stress(d):
    run(*tb.stress_table(d), 65, 65)


WRAPPED = [(d, k) for d in (8, 40) for k in (65, 1023)]


@pytest.mark.parametrize("d, k", WRAPPED, ids=[f"d{d}-k{k}" for d, k in WRAPPED])
def test_wrapper_takes_the_prefilter(d, k, monkeypatch):
    from muygpys_amd import _lib
    from muygpys_amd.neighbors import NN_Wrapper

    for name in ("MUYGPYS_HIP_KNN_WIDE", "MUYGPYS_HIP_KNN_LONG", "MUYGPYS_HIP_KNN_PAD"):
        monkeypatch.delenv(name, raising=False)
    X, Q, bi = tw.wrapper_problem(9001, d)
    auto, nn = NN_Wrapper(X, k), NN_Wrapper(X, k, scan_kind="prefilter")
    calls, real = [], _lib.load().mgp_knn_scan_wide_bf16x3
    monkeypatch.setattr(_lib.load(), "mgp_knn_scan_wide_bf16x3", lambda *a: calls.append(1) or real(*a))
    for pts, exclude in ((nn._pad_features(Q - nn._mean), None), (nn.train[nn._inv[bi]], bi)):
        (wi, wd), (ai, _) = ((w.get_nns(Q) if exclude is None else w.get_batch_nns(bi)) for w in (nn, auto))
        assert nn.last_route == auto.last_route == "wide"
        D, scale = tw.wrapper_reference(nn, pts, exclude)
        clear = tw.check_wrapper_answer(wi, wd, D, scale, d, k, exclude)
        assert torch.equal(wi[clear], ai[clear])
    assert len(calls) == 2, "mgp_knn_scan_wide_bf16x3 served both searches, and only the prefilter object's"


@pytest.mark.parametrize("d, k, route", [(40, 30, "scan"), (100, 65, "long")])
def test_other_shapes_do_not_reach_the_entry(d, k, route, monkeypatch):
    from muygpys_amd import _lib
    from muygpys_amd.neighbors import NN_Wrapper

    X, Q, _ = tw.wrapper_problem(9001, d)
    calls, real = [], _lib.load().mgp_knn_scan_wide_bf16x3
    monkeypatch.setattr(_lib.load(), "mgp_knn_scan_wide_bf16x3", lambda *a: calls.append(1) or real(*a))
    nn = NN_Wrapper(X, k, scan_kind="prefilter")
    nn.get_nns(Q)
    assert nn.last_route == route and not calls
