"""GPU: the three exact k-NN scans of the C ABI, called directly at the shape edges NN_Wrapper never reaches (it
refuses tables of 8 192 rows or fewer and always starts at a multiple of 1 024), against fp64 brute force.

Entries and the instantiation a feature count d selects (csrc/mgp_knn.hip, the two `switch` statements):

    mgp_knn_scan_f32         launch_knn_dp<DP>, DP = 8 ceil(d / 8)
        d = 4, 8 -> DP 8     12 -> 16     20 -> 24     28, 32 -> 32     40 -> 40     44, 48 -> 48     52, 56 -> 56
        60, 64 -> 64         (d % 8 == 4: half of the wave's last 16-byte group is zero padding)
    mgp_knn_scan_bf16x3      launch_knn_packed_kp<KP, 2>, KP = 16 ceil((d + 2) / 16): the row width changes at d + 2
        d = 4, 8, 12 -> KP 16 (128-row swizzled tile)     16, 24, 28 -> 32     32, 40, 44 -> 48     48, 60 -> 64
        64 -> 80
    mgp_knn_scan_bf16x2_d8   launch_knn_packed_kp<8, 2> (d = 4, 8), and launch_knn_packed_kp<8, 4> with
                             MUYGPYS_HIP_KNN_RB4_MIN=0 (the entry called "d8rb4" below)

Tiles are TN = 128 rows for the packed entries at d + 2 <= 16 and for the d8 layout, 64 otherwise; a workgroup owns
QB = 128 (f32), 256 (packed, two row blocks) or 512 (four row blocks) queries.

What a call is made of (`run_scan`): the table centred on its fp64 mean (queries shifted alike), squared norms rounded
from fp64 and padded with +inf to a multiple of 64, IN lists = the exact k-best over rows [0, start) from torch (Gram
form fp32 for the f32 entry, difference form fp32 for the packed ones), packed rows from NN_Wrapper's own pack helpers
with its c and QMAX = 1.25 max|q|, a zero-filled overflow vector.  The result is the entry's unordered lists.

Reference and bound (`check`): fp64 distances on the same (centred fp32) data, self excluded.  Per query the fp64
distances of the returned rows, sorted, are compared element by element with the sorted true top-k.  A selection that
is exact under distances perturbed by at most e returns sorted true distances within 2 e of the true top-k, with
    packed entries   e = (d + 2) 2^-24 dist   (fp32 difference form: a rounded difference, its square, d - 1 additions)
    f32 entry        e = (d + 5) 2^-24 (|q|^2 + max_x |x|^2)   (Gram form: an fmaf chain of d products from -|x|^2/2,
                     fp32-rounded norms)
The largest 2 e any case here uses: 7.9e-6 relative (packed, d = 64), 1.7e-3 absolute on squared distances of
60 to 130 (f32, d = 64); the gaps between order statistics at these sizes are 1e-2 to 1e-3 relative.

No overflow in the benign cases is a property of the inputs, asserted in fp64 before the kernel's flags are looked at
(`assert_queues_cannot_overflow`): the thresholds only tighten, so what can enter a query's 16-entry queue between
two drains is a subset of the rows of that window closer than the query's k-th best over [0, start) -- at most 12 in
every window of tiles a workgroup of the case drains together.  start = max(64, TN k / 2 rounded up to 64) makes that
hold with room to spare (NN_Wrapper's sizing without its 1 024-row floor)."""

import types
import zlib

import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

U = 2.0 ** -24          # unit roundoff of fp32
QUEUE_ROOM = 12         # of the 16 queue entries; four are head-room for pre-filter near misses

ENTRIES = ("f32", "x3", "d8", "d8rb4")
SYMBOL = {"f32": "mgp_knn_scan_f32", "x3": "mgp_knn_scan_bf16x3", "d8": "mgp_knn_scan_bf16x2_d8",
          "d8rb4": "mgp_knn_scan_bf16x2_d8"}
QUERY_BLOCK = {"f32": 128, "x3": 256, "d8": 256, "d8rb4": 512}


def tile_rows(entry, d):
    return 128 if entry in ("d8", "d8rb4") or (entry == "x3" and d + 2 <= 16) else 64


def instantiation(entry, d):
    if entry == "f32":
        return f"DP{(d + 7) // 8 * 8}"
    if entry == "x3":
        return f"KP{(d + 2 + 15) // 16 * 16}"
    return "KP8xRB2" if entry == "d8" else "KP8xRB4"


def case_id(entry, d, *rest):
    return "-".join([entry, f"d{d}", instantiation(entry, d), *map(str, rest)])


def start_rows(k, tn):
    return max(64, -(-(tn * k // 2) // 64) * 64)


def drain_windows(entry, tn, start, ntiles, block):
    """The tiles workgroup `block` drains together, in walk order: the kernels' own rules -- the start tile of the
    staggered walk, and the interval between two drains (the last tile always drains)."""
    first = block * 7919 % ntiles if entry == "f32" else block % 64 % ntiles
    windows, current, next_drain = [], [], 0
    for tj in range(ntiles):
        current.append((first + tj) % ntiles)
        if tj < next_drain and tj + 1 < ntiles:
            continue
        if entry == "f32":
            step = 1 if tj < 64 else 4 if tj < 256 else 8 if tj < 1024 else 16
        else:
            every = min(max((start + tj * tn) // 64, 64), 16384)
            step = max(every // tn, 1)
        next_drain = tj + step
        windows.append(current)
        current = []
    return windows


@pytest.fixture
def select(monkeypatch):
    """Chooses the row-block form of the d8 entry (its launcher reads the variable on every call)."""
    def _select(entry):
        if entry == "d8rb4":
            monkeypatch.setenv("MUYGPYS_HIP_KNN_RB4_MIN", "0")
        else:
            monkeypatch.delenv("MUYGPYS_HIP_KNN_RB4_MIN", raising=False)
    return _select


# cases whose first draw broke the no-overflow precondition (a query with an unlucky head sample meets more than 12
# closer rows in one tile): another seed, the same cap
RESEED = {"d/d8/8/1/130/137/64": 1, "d/x3/16/2/130/73/64": 1}


def normal(seed_of, n, d, m):
    g = torch.Generator().manual_seed(zlib.crc32(f"{seed_of}#{RESEED.get(seed_of, 0)}".encode()))
    return torch.randn(n, d, generator=g).cuda(), torch.randn(m, d, generator=g).cuda()


def run_scan(entry, X, Q, k, start, self_idx=None, qmax_factor=1.25):
    """One direct call of an entry; returns the centred data, the unordered lists and the overflow flags."""
    from muygpys_amd import _lib
    from muygpys_amd.neighbors import NN_Wrapper

    mean = X.double().mean(0)
    Xc = (X.double() - mean).float().contiguous()
    Qc = (Q.double() - mean).float().contiguous()
    (n, d), m = Xc.shape, Qc.shape[0]
    assert k + 1 <= start < n and start % 4 == 0
    sq = (Xc.double() ** 2).sum(1).float()
    sqn = torch.cat([sq, torch.full(((-n) % 64,), float("inf"), device=sq.device)])
    qn = (Qc.double() ** 2).sum(1).float()
    head = Xc[:start]
    best_d = torch.empty((m, k), device=Xc.device, dtype=torch.float32)
    best_i = torch.empty((m, k), device=Xc.device, dtype=torch.int32)
    step = max(1, (1 << 24) // (start * d))
    for s in range(0, m, step):
        qq = Qc[s:s + step]
        if entry == "f32":
            d2 = sq[None, :start] - 2.0 * (qq @ head.T) + qn[s:s + step, None]
        else:
            diff = qq[:, None, :] - head[None]
            d2 = (diff * diff).sum(-1)
        if self_idx is not None:
            ex = self_idx[s:s + step]
            inside = ex < start
            d2[torch.arange(qq.shape[0], device=ex.device)[inside], ex[inside]] = float("inf")
        bd, bi = d2.topk(k, dim=1, largest=False)
        best_d[s:s + step], best_i[s:s + step] = bd, bi.to(torch.int32)
    assert bool(torch.isfinite(best_d).all()), "the IN lists must be finite (start >= k + 1)"
    overflow = torch.zeros((m,), device=Xc.device, dtype=torch.int32)
    ex64 = None if self_idx is None else self_idx.to(torch.int64).contiguous()
    fn = getattr(_lib.load(), SYMBOL[entry])
    if entry == "f32":
        rc = fn(_lib.ptr(Xc), _lib.ptr(sqn), n, d, _lib.ptr(Qc), _lib.ptr(qn), _lib.ptr(ex64), m, k, start,
                _lib.ptr(best_d), _lib.ptr(best_i), _lib.ptr(overflow), _lib.stream_ptr())
    else:
        qmax = qmax_factor * float(qn.max().sqrt())
        c = -0.5 * sq + (2.0 ** -14 * qmax) * sq.sqrt()
        c = c + 2.0 ** -15 * c.abs()
        pack = NN_Wrapper._pack_bf16 if entry == "x3" else NN_Wrapper._pack_bf16_d8
        packed_train, packed_q = pack(Xc, c, 1.0).contiguous(), pack(Qc, 1.0, 0.0).contiguous()
        rc = fn(_lib.ptr(Xc), _lib.ptr(packed_train), _lib.ptr(sqn), n, d, _lib.ptr(Qc), _lib.ptr(packed_q), _lib.ptr(qn),
                _lib.ptr(ex64), m, k, start, _lib.ptr(best_d), _lib.ptr(best_i), _lib.ptr(overflow), _lib.stream_ptr())
    assert rc == 0, (SYMBOL[entry], rc)
    torch.cuda.synchronize()
    return types.SimpleNamespace(entry=entry, X=Xc, Q=Qc, n=n, d=d, m=m, k=k, start=start, self_idx=self_idx,
                                 best_d=best_d, best_i=best_i, overflow=overflow)


def true_distances(r):
    """(m, n) fp64 squared distances of the call's data, +inf at a query's own row.  Computed once per case."""
    D = torch.cdist(r.Q.double(), r.X.double(), compute_mode="donot_use_mm_for_euclid_dist") ** 2
    if r.self_idx is not None:
        D[torch.arange(r.m, device=D.device), r.self_idx] = float("inf")
    return D


def assert_queues_cannot_overflow(r, D):
    """The precondition of `overflow.sum() == 0`, from the inputs alone (see the module docstring)."""
    tn = tile_rows(r.entry, r.d)
    ntiles = -(-(r.n - r.start) // tn)
    tau0 = D[:, :r.start].topk(r.k, dim=1, largest=False).values[:, -1]
    beats = (D[:, r.start:] < tau0[:, None]).to(torch.int32)
    beats = torch.nn.functional.pad(beats, (0, ntiles * tn - beats.shape[1]))
    per_tile = beats.reshape(r.m, ntiles, tn).sum(-1)
    qb = QUERY_BLOCK[r.entry]
    worst = longest = 0
    for block in range(-(-r.m // qb)):
        mine = per_tile[block * qb:(block + 1) * qb]
        for window in drain_windows(r.entry, tn, r.start, ntiles, block):
            worst, longest = max(worst, int(mine[:, window].sum(1).max())), max(longest, len(window))
    assert worst <= QUEUE_ROOM, (f"{worst} rows of one drain window beat a query's initial k-th best: change the seed "
                                 f"of {getattr(r, 'seed_of', 'this case')!r}")
    return longest


def check_lists(r, D):
    """Rows in range, distinct, never self.  (Holds for flagged queries too.)"""
    bi = r.best_i.long()
    assert int(bi.min()) >= 0 and int(bi.max()) < r.n, (int(bi.min()), int(bi.max()), r.n)
    rows = bi.sort(dim=1).values
    assert bool((rows[:, 1:] != rows[:, :-1]).all()), "a row twice in one list"
    if r.self_idx is not None:
        assert not bool((bi == r.self_idx[:, None]).any()), "a query's own row was returned"
    return bi


def check(r, D=None):
    """Everything a benign case asserts; returns the lists as int64."""
    D = true_distances(r) if D is None else D
    w = assert_queues_cannot_overflow(r, D)
    bi = check_lists(r, D)
    got = D.gather(1, bi)
    want = D.topk(r.k, dim=1, largest=False).values  # ascending
    got_sorted = got.sort(dim=1).values
    if r.entry == "f32":
        scale = (r.Q.double() ** 2).sum(1) + (r.X.double() ** 2).sum(1).max()
        e_own = e_pair = ((r.d + 5) * U * scale)[:, None].expand(r.m, r.k)
    else:
        e_own = (r.d + 2) * U * torch.maximum(got, r.best_d.double())
        e_pair = (r.d + 2) * U * torch.maximum(got_sorted, want)
    own = (r.best_d.double() - got).abs()
    pair = (got_sorted - want).abs()
    print(f"\n[{r.entry} d={r.d} k={r.k} m={r.m} n={r.n} start={r.start} drain window {w} tile(s)] "
          f"largest 2e {float((2 * e_pair).max()):.3e} (relative {float((2 * e_pair / want.clamp(min=1e-300)).max()):.3e}), "
          f"sorted distances off by at most {float(pair.max()):.3e}, best_d by {float(own.max()):.3e}, "
          f"flagged {int(r.overflow.sum())}")
    assert bool((own <= e_own).all()), f"best_d is not the distance of its row: off by {float((own - e_own).max()):.3e} past e"
    assert bool((pair <= 2 * e_pair).all()), (
        f"a true neighbour is missing: {int((pair > 2 * e_pair).any(1).sum())} of {r.m} queries, "
        f"worst {float((pair - 2 * e_pair).max()):.3e} past 2e")
    assert int(r.overflow.sum()) == 0, f"{int(r.overflow.sum())} of {r.m} queries flagged on inputs that cannot overflow"
    return bi


def benign(entry, d, k, m, past_start, select, name, start=None, **scan):
    select(entry)
    tn = tile_rows(entry, d)
    start = start_rows(k, tn) if start is None else start
    seed_of = f"{name}/{entry}/{d}/{k}/{m}/{past_start}/{start}"
    X, Q = normal(seed_of, start + past_start, d, m)
    r = run_scan(entry, X, Q, k, start, **scan)
    r.seed_of = seed_of
    check(r)
    return r


# ---- (a) every instantiation ---------------------------------------------------------------------------------------
INSTANCES = ([("f32", d) for d in (4, 8, 12, 20, 28, 32, 40, 44, 48, 52, 56, 60, 64)]
             + [("x3", d) for d in (4, 12, 16, 28, 32, 44, 48, 60, 64)]
             + [(e, d) for e in ("d8", "d8rb4") for d in (4, 8)])


@pytest.mark.parametrize("entry, d", INSTANCES, ids=[case_id(e, d) for e, d in INSTANCES])
def test_every_instantiation(entry, d, select):
    benign(entry, d, 10, 300, 3 * tile_rows(entry, d) + 5, select, "a")


# ---- (b) table edges -----------------------------------------------------------------------------------------------
EDGE_SHAPES = (("x3", 12), ("x3", 40), ("d8", 8), ("d8rb4", 8), ("f32", 40))


def _table_edges():
    out = []
    for entry, d in EDGE_SHAPES:
        tn = tile_rows(entry, d)
        for past, what in ((1, "1row"), (tn - 1, "TN-1"), (tn, "TN"), (tn + 1, "TN+1"), (2 * tn + 3, "2TN+3")):
            out.append((entry, d, past, None, what))
        if entry == "f32":
            # past tj = 64 the drain interval is four tiles -- at 70 tiles already (steps 65 to 68), and a workgroup that
            # started late meets the FIRST rows of the table there: 256 rows behind a start of 320 bring six rows per
            # query on average, behind 1 024 two.  Both long walks of this entry start at 1 024
            out += [(entry, d, 70 * tn - 5, 1024, "70tiles-start1024"), (entry, d, 80 * tn - 5, 1024, "80tiles-start1024")]
        else:  # (one tile between two drains at these sizes); the packed entries also take a start off the tile grid
            s = start_rows(10, tn)
            out += [(entry, d, 70 * tn - 5, None, "70tiles"),
                    (entry, d, 2 * tn + 3, s + 4, "start+4"), (entry, d, 2 * tn + 3, s + 68, "start+68")]
    return out


@pytest.mark.parametrize("entry, d, past, start, what", _table_edges(),
                         ids=[case_id(e, d, w) for e, d, _, _, w in _table_edges()])
def test_table_edges(entry, d, past, start, what, select):
    r = benign(entry, d, 10, 600, past, select, "b", start=start)
    if "tiles" in what:  # the walk is as long as the case says, and the f32 one reaches the four-tile interval
        tn = tile_rows(entry, d)
        ntiles = -(-(r.n - r.start) // tn)
        assert ntiles == int(what[:2]) > 64
        longest = max(len(w) for b in range(5) for w in drain_windows(entry, tn, r.start, ntiles, b))
        assert longest == (4 if entry == "f32" else 1)


# ---- (c) query-count edges -----------------------------------------------------------------------------------------
def _query_edges():
    out = []
    for entry, d in (("f32", 8), ("f32", 40), ("x3", 8), ("x3", 40), ("d8", 8), ("d8rb4", 8)):
        qb = QUERY_BLOCK[entry]
        out += [(entry, d, m, what) for m, what in ((1, "m1"), (qb - 1, "QB-1"), (qb, "QB"), (qb + 1, "QB+1"),
                                                    (2 * qb + 3, "2QB+3"))]
    return out


@pytest.mark.parametrize("entry, d, m, what", _query_edges(), ids=[case_id(e, d, w) for e, d, _, w in _query_edges()])
def test_query_count_edges(entry, d, m, what, select):
    benign(entry, d, 10, m, 2 * tile_rows(entry, d) + 7, select, "c")


# ---- (d) k edges ---------------------------------------------------------------------------------------------------
K_EDGES = [(e, d, k) for e, d in (("f32", 16), ("x3", 16), ("d8", 8), ("d8rb4", 8))
           for k in (1, 2, 15, 16, 17, 32, 33, 48, 49, 63, 64)]


@pytest.mark.parametrize("entry, d, k", K_EDGES, ids=[case_id(e, d, f"k{k}") for e, d, k in K_EDGES])
def test_k_edges(entry, d, k, select):
    r = benign(entry, d, k, 130, tile_rows(entry, d) + 9, select, "d")
    assert r.start <= 4096 and r.start >= k + 1


# ---- (e) self exclusion and duplicates -----------------------------------------------------------------------------
SELF_SHAPES = [("f32", 8), ("f32", 40), ("x3", 8), ("x3", 40), ("d8", 8), ("d8rb4", 8)]


@pytest.mark.parametrize("entry, d", SELF_SHAPES, ids=[case_id(e, d) for e, d in SELF_SHAPES])
def test_self_exclusion_and_duplicates(entry, d, select):
    """Queries are table rows, half below `start` and half past it, each with an exact copy planted elsewhere past
    `start`: the copy comes back at distance 0, the row itself never."""
    select(entry)
    k, m, tn = 10, 64, tile_rows(entry, d)
    start = start_rows(k, tn)
    n = start + 4 * tn + 5
    X, _ = normal(f"e/{entry}/{d}", n, d, 1)
    g = torch.Generator().manual_seed(d)
    below = torch.randperm(start, generator=g)[:m // 2]
    past = start + torch.randperm(n - start, generator=g)[:m // 2 + m]  # (the second half's own rows, then the copies)
    self_idx = torch.cat([below, past[:m // 2]]).cuda()
    copy = past[m // 2:].cuda()
    X[copy] = X[self_idx]
    r = run_scan(entry, X, X[self_idx].clone(), k, start, self_idx=self_idx)
    assert torch.equal(r.X[copy], r.Q)  # (centring kept the copies exact)
    D = true_distances(r)
    bi = check(r, D)
    hit = bi == copy[:, None]
    assert bool(hit.any(1).all()), "a planted copy is missing"
    assert bool((D.gather(1, bi)[hit] == 0).all())
    if entry != "f32":  # (difference form: exactly zero; the Gram form is held to e by `check`)
        assert bool((r.best_d[hit] == 0).all())


# ---- (f) scale (packed rows) ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["x1e3", "x1e-3", "spreads", "qmax"])
@pytest.mark.parametrize("d", [12, 44])
def test_packed_rows_at_other_scales(d, what, select):
    """The pre-filter's margin is relative to |q| |x|: nothing changes at another scale, with per-feature spreads from
    1e-2 to 1e2, or when a query's norm equals the QMAX the table was packed for."""
    entry = "x3"
    select(entry)
    k, m, tn = 10, 300, tile_rows(entry, d)
    start = start_rows(k, tn)
    X, Q = normal(f"f/{d}/{what}", start + 3 * tn + 5, d, m)
    if what.startswith("x"):
        X, Q = X * float(what[1:]), Q * float(what[1:])
    if what == "spreads":
        s = torch.logspace(-2, 2, d, device=X.device)
        X, Q = X * s, Q * s
    r = run_scan(entry, X, Q, k, start, qmax_factor=1.0 if what == "qmax" else 1.25)
    check(r)


# ---- (g) placement invariance --------------------------------------------------------------------------------------
PLACED = [("f32", 24), ("x3", 24), ("d8", 8), ("d8rb4", 8)]


@pytest.mark.parametrize("entry, d", PLACED, ids=[case_id(e, d) for e, d in PLACED])
def test_placement_invariance(entry, d, select):
    """The same queries in another order (other workgroups, lanes and start tiles) return the same row sets."""
    select(entry)
    k, m, tn = 10, 600, tile_rows(entry, d)
    start = start_rows(k, tn)
    X, Q = normal(f"g/{entry}/{d}", start + 5 * tn + 3, d, m)
    order = torch.randperm(m, generator=torch.Generator().manual_seed(7)).cuda()
    a = run_scan(entry, X, Q, k, start)
    b = run_scan(entry, X, Q[order].contiguous(), k, start)
    rows_a = check(a).sort(dim=1).values
    rows_b = check(b).sort(dim=1).values
    assert torch.equal(rows_a[order], rows_b)


# ---- (h) adversarial order -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ENTRIES, ids=[case_id(e, 8) for e in ENTRIES])
def test_adversarial_order_flags_every_query(entry, select):
    """All queries at the origin, the table sorted farthest first: every row beats every earlier one, so each drain
    meets a whole tile of candidates in a 16-entry queue.  Every query is flagged -- by construction, not by chance;
    the flagged lists are incomplete by contract, but hold distinct rows of the table."""
    select(entry)
    d, k, m, tn = 8, 10, 200, tile_rows(entry, 8)
    start = start_rows(k, tn)
    X, _ = normal(f"h/{entry}", start + 4 * tn, d, 1)
    X = (X.double() - X.double().mean(0)).float()
    X = X[(X.double() ** 2).sum(1).argsort(descending=True)].contiguous()
    Q = X.double().mean(0).float().expand(m, d).contiguous()  # (the origin once the call has centred it)
    self_idx = torch.arange(m, device=X.device) * (X.shape[0] // m)  # (rows on both sides of start)
    r = run_scan(entry, X, Q, k, start, self_idx=self_idx)
    D = true_distances(r)
    # the construction: in every tile at least 17 rows are closer than the initial k-th best of every query
    tau0 = D[:, :start].topk(k, dim=1, largest=False).values[:, -1]
    per_tile = (D[:, start:] < tau0[:, None]).reshape(m, 4, tn).sum(-1)
    assert int(per_tile.min()) >= tn - 1 > 16
    check_lists(r, D)
    assert bool((r.overflow == 1).all()), f"{int((r.overflow == 0).sum())} of {m} queries not flagged"
