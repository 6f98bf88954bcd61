"""GPU: the per-function tensor kernels of csrc/mgp_tensor_ops.hip through the C ABI, every launch route and both
sides of every grid cap, against exact or derivation-bounded references.

Cases, routes, references and bounds: tests/tensor_ops_cases.py (its docstring derives every bound); that every route
and cap is reached: tests/test_tensor_ops_cases_cpu.py.  The entries are called directly: the Python wrappers cannot
hand over a pointer that is not 16-byte aligned, nor a NULL batch_idx.

What every case asserts (`Call`): the status is MGP_OK; the output lies between 64 sentinel elements on either side
in a buffer pre-filled with NaN, the sentinels keep their bits and no NaN remains where the reference has none; every
input keeps its bits; the result meets its entry's bound (error / bound <= 1; exact entries: equal bytes).  A pointer
"off by one element" is a view one element into a torch allocation: element-aligned, not 16-byte aligned.

Worst observed error / bound per entry and dtype on an MI355X (measurements; they decide nothing):

    entry             fp32     fp64
    crosswise_diffs   exact    exact
    pairwise_diffs    exact    exact
    crosswise_dists   0.581    0.564
    reduce_diffs      0.361    0.332
    pairwise_dists    0.623    0.724
    kernel_apply      0.642    0.762
    perturb           exact    exact
    loss_sums         0.128    0.090
    column_sums       0.000    0.016    (fp32 columns of these sizes add without a rounding in fp64)
    table_pack        exact    exact

`test_zz_report_worst_ratios` prints this table from a run (python -m pytest -s)."""

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests import tensor_ops_cases as tc  # noqa: E402

TORCH_DTYPE = {"f32": torch.float32, "f64": torch.float64}
BITS = {torch.float32: torch.int32, torch.float64: torch.int64}
RATIOS = {}


def ids(cases):
    return [c.id for c in cases]


def entry_fn(c):
    from muygpys_amd import _lib

    return getattr(_lib.load(), f"mgp_{c.entry}_{c.dtype}")


def dev_in(arr, mis=False):
    """An input on the device: 16-byte aligned, or one element past a 16-byte boundary."""
    if arr is None:
        return None
    flat = torch.from_numpy(np.ascontiguousarray(arr).reshape(-1))
    t = torch.empty(flat.numel() + 1, dtype=flat.dtype, device="cuda")
    v = t[1:] if mis else t[:-1]
    v.copy_(flat)
    assert v.data_ptr() % 16 == (flat.element_size() if mis else 0)
    return v


class Guarded:
    """`numel` elements between sentinels, everything NaN before the call."""

    def __init__(self, numel, dtype, mis=False):
        self.lead = tc.GUARD + (1 if mis else 0)
        self.numel = numel
        self.buf = torch.full((self.lead + numel + tc.GUARD,), float("nan"), dtype=dtype, device="cuda")
        self.view = self.buf[self.lead:self.lead + numel]
        assert self.view.data_ptr() % 16 == (self.buf.element_size() if mis else 0)
        self.before = self._guards()

    def _guards(self):
        bits = self.buf.view(BITS[self.buf.dtype])
        return torch.cat([bits[:self.lead], bits[self.lead + self.numel:]]).clone()

    def intact(self):
        return torch.equal(self._guards(), self.before)

    def untouched(self):
        return self.intact() and bool(torch.isnan(self.view).all())

    def numpy(self):
        return self.view.cpu().numpy()


class Call:
    """One call of an entry: the inputs of a case on the device, the guarded output, the checks every case shares."""

    def __init__(self, c, s, out_numel, out_dtype=None):
        self.c, self.s = c, s
        self.inputs = {}
        self.out = Guarded(out_numel, out_dtype or TORCH_DTYPE[c.dtype], mis="out" in c.mis)

    def put(self, name):
        arr = getattr(self.s, name)
        t = dev_in(arr, mis=name in self.c.mis)
        if arr is not None:
            self.inputs[name] = (arr, t)
        return t

    def run(self, *args, expect=0):
        from muygpys_amd import _lib

        ptr = lambda a: _lib.ptr(a) if a is None or isinstance(a, torch.Tensor) else a
        rc = entry_fn(self.c)(*[ptr(a) for a in args], _lib.stream_ptr())
        torch.cuda.synchronize()
        assert rc == expect, (self.c.id, rc)
        assert self.out.intact(), f"{self.c.id}: a sentinel next to the output changed"
        for name, (arr, t) in self.inputs.items():
            assert t.cpu().numpy().tobytes() == np.ascontiguousarray(arr).tobytes(), f"{self.c.id}: input {name} changed"
        return self.out.numpy()


def assert_exact(c, got, want):
    want = np.ascontiguousarray(want).reshape(-1)
    assert got.dtype == want.dtype and got.shape == want.shape
    if got.tobytes() != want.tobytes():
        bad = np.flatnonzero(got.view(f"u{got.itemsize}") != want.view(f"u{want.itemsize}"))
        raise AssertionError(f"{c.id}: {bad.size} of {got.size} elements differ, first at {bad[0]}: got {got[bad[0]]!r}, "
                             f"want {want[bad[0]]!r}")
    RATIOS.setdefault((c.entry, c.dtype), 0.0)


def assert_bounded(c, got, ref, bound, what=""):
    """error / bound <= 1 everywhere (a zero bound asks for the exact value); records the worst ratio."""
    ref = np.asarray(ref).reshape(-1)
    bound = np.asarray(bound).reshape(-1)
    err = np.abs(got.reshape(-1).astype(ref.dtype) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))
    worst = float(ratio.max())
    key = (c.entry, c.dtype)
    RATIOS[key] = max(RATIOS.get(key, 0.0), worst) if worst == worst else float("nan")
    print(f"\n[{c.id}{' ' + what if what else ''}] route {tc.case_route(c)}, worst error / bound {worst:.3f}")
    if not worst <= 1.0:
        at = int(np.nanargmax(np.where(np.isnan(ratio), np.inf, ratio)))
        raise AssertionError(f"{c.id} {what}: error / bound {worst:.3f} at flat index {at}: got {got.reshape(-1)[at]!r}, "
                             f"reference {ref[at]!r}, bound {bound[at]!r}")


# ---- differences: exact -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", tc.cases_of("crosswise_diffs"), ids=ids(tc.cases_of("crosswise_diffs")))
def test_crosswise_diffs(c):
    s = tc.make_inputs(c)
    call = Call(c, s, c.b * c.k * c.d)
    got = call.run(call.put("fq"), call.put("fn"), c.d, call.put("bidx"), call.put("nidx"), c.b, c.k, call.out.view)
    assert_exact(c, got, tc.ref_crosswise_diffs(s.fq, s.fn, s.bidx, s.nidx))


@pytest.mark.parametrize("c", tc.cases_of("pairwise_diffs"), ids=ids(tc.cases_of("pairwise_diffs")))
def test_pairwise_diffs(c):
    s = tc.make_inputs(c)
    call = Call(c, s, c.b * c.k * c.k * c.d)
    got = call.run(call.put("f"), c.d, call.put("nidx"), c.b, c.k, call.out.view)
    assert_exact(c, got, tc.ref_pairwise_diffs(s.f, s.nidx))


# ---- distances ------------------------------------------------------------------------------------------------------------------

def metric_id(c):
    from muygpys_amd import _lib

    return _lib.METRIC_IDS[c.metric]


@pytest.mark.parametrize("c", tc.cases_of("crosswise_dists"), ids=ids(tc.cases_of("crosswise_dists")))
def test_crosswise_dists(c):
    s = tc.make_inputs(c)
    call = Call(c, s, c.b * c.k)
    got = call.run(call.put("fq"), call.put("fn"), c.d, call.put("bidx"), call.put("nidx"), c.b, c.k, metric_id(c),
                   call.out.view)
    assert_bounded(c, got, *tc.ref_crosswise_dists(c, s))


@pytest.mark.parametrize("c", tc.cases_of("reduce_diffs"), ids=ids(tc.cases_of("reduce_diffs")))
def test_reduce_diffs(c):
    s = tc.make_inputs(c)
    call = Call(c, s, c.n)
    got = call.run(call.put("diffs"), c.n, c.d, call.put("ls"), metric_id(c), call.out.view)
    assert_bounded(c, got, *tc.ref_reduce_diffs(c, s))


def run_pairwise_dists(c, s):
    call = Call(c, s, c.b * c.k * c.k)
    return call.run(call.put("f"), c.d, call.put("nidx"), c.b, c.k, metric_id(c), call.out.view).reshape(c.b, c.k, c.k)


@pytest.mark.parametrize("c", tc.cases_of("pairwise_dists"), ids=ids(tc.cases_of("pairwise_dists")))
def test_pairwise_dists(c):
    s = tc.make_inputs(c)
    got = run_pairwise_dists(c, s)
    ref, bound = tc.ref_pairwise_dists(c, s)
    assert_bounded(c, got, ref, bound)
    i = np.arange(c.k)
    assert not got[:, i, i].any(), "a diagonal entry is not exactly 0"
    assert got.tobytes() == np.ascontiguousarray(got.transpose(0, 2, 1)).tobytes(), "out[b, i, j] and out[b, j, i] differ in bits"
    same = s.nidx[:, :, None] == s.nidx[:, None, :]
    if c.k >= 3:
        assert same[0, 1, 2], "the case's repeated neighbour"
    assert not got[same].any(), "a repeated neighbour is not at distance exactly 0"


def one_of_each_pairwise_route(dtype):
    """A small case of every kernel body and gather form: both NP in vec and scalar form at 1 and 4 blocks, tile, thread."""
    picked = {}
    for c in tc.cases_of("pairwise_dists"):
        r = tc.case_route(c)
        if c.dtype == dtype and c.k >= 3 and c.b <= 3 and ("_s2_" not in r and "_s3_" not in r) and r not in picked:
            picked[r] = c
    return list(picked.values())


NAN_CASES = one_of_each_pairwise_route("f32") + one_of_each_pairwise_route("f64")


@pytest.mark.parametrize("c", NAN_CASES, ids=ids(NAN_CASES))
def test_pairwise_dists_nan_row_poisons_its_row_and_column_only(c):
    s = tc.make_inputs(c)
    # distinct neighbours, so that the poisoned table row sits at one place per neighbourhood
    rng = np.random.default_rng(c.k)
    s.nidx = np.stack([rng.permutation(max(tc.TABLE_ROWS, c.k))[:c.k] for _ in range(c.b)]).astype(np.int64)
    if c.k > tc.TABLE_ROWS:
        s.f = rng.standard_normal((c.k, c.d)).astype(s.f.dtype)
    poisoned = int(s.nidx[0, c.k // 2])
    s.f[poisoned, c.d - 1] = np.nan  # the LAST feature: a kernel that skips it forgets the NaN
    got = run_pairwise_dists(c, s)
    at = s.nidx == poisoned
    want = at[:, :, None] | at[:, None, :]
    assert want[0].any() and not want[0].all()
    assert np.array_equal(np.isnan(got), want), f"{tc.case_route(c)}: NaN at {int(np.isnan(got).sum())} places, expected {int(want.sum())}"


VEC_SHAPES = [c for c in tc.cases_of("pairwise_dists") if tc.case_route(c).endswith("_vec") and c.b <= 3 and c.k in (31, 32, 33, 63)]


@pytest.mark.parametrize("c", VEC_SHAPES, ids=ids(VEC_SHAPES))
def test_pairwise_dists_vector_and_scalar_gather_each_meet_the_bound(c):
    """The same inputs through the 16-byte gather (f aligned) and the scalar gather (f one element off): each within the
    bound of the reference -- they are not compared with each other."""
    s = tc.make_inputs(c)
    ref, bound = tc.ref_pairwise_dists(c, s)
    assert_bounded(c, run_pairwise_dists(c, s), ref, bound, "vec")
    c2 = tc.make_case("pairwise_dists", c.dtype, d=c.d, k=c.k, b=c.b, metric=c.metric, mis=("f",))
    assert tc.case_route(c2) == tc.case_route(c).replace("_vec", "_scalar")
    assert_bounded(c2, run_pairwise_dists(c2, s), ref, bound, "scalar, the inputs of " + c.id)


# ---- kernel functions -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", tc.cases_of("kernel_apply"), ids=ids(tc.cases_of("kernel_apply")))
def test_kernel_apply(c):
    from muygpys_amd import _lib

    s = tc.make_inputs(c)
    call = Call(c, s, c.n)
    got = call.run(call.put("x"), c.n, _lib.KERNEL_IDS[c.kernel], float(c.scale), call.out.view)
    ref, bound, inside = tc.ref_kernel_apply(c, s)
    assert inside.any()
    assert_bounded(c, got[inside], ref[inside], bound[inside])
    beyond = got[~inside].astype(ref.dtype)
    assert np.all(np.isfinite(beyond)) and np.all(beyond >= 0) and np.all(beyond <= tc.ref_kernel_end(c)), beyond


# ---- nugget ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", tc.cases_of("perturb"), ids=ids(tc.cases_of("perturb")))
def test_perturb(c):
    from muygpys_amd import _lib

    s = tc.make_inputs(c)
    call = Call(c, s, c.b * c.k * c.k)
    mode = _lib.NOISE_SCALAR if c.mode == "scalar" else _lib.NOISE_BATCH
    got = call.run(call.put("Kin"), c.b, c.k, mode, float(s.eps), call.put("noise"), call.out.view)
    assert_exact(c, got, tc.ref_perturb(c, s))


# ---- fp64 reductions ------------------------------------------------------------------------------------------------------------

def guarded_scratch(fill):
    g = Guarded(tc.SCRATCH_DOUBLES, torch.float64)
    g.view.fill_(fill)
    return g


@pytest.mark.parametrize("c", tc.cases_of("loss_sums"), ids=ids(tc.cases_of("loss_sums")))
def test_loss_sums(c):
    from muygpys_amd import _lib

    assert _lib.load().mgp_reduce_scratch_doubles() == tc.SCRATCH_DOUBLES
    s = tc.make_inputs(c)
    ref, bound = tc.ref_loss_sums(c, s)
    runs = []
    for fill in (0.0, float("nan")) if c.scratch else (None,):
        call = Call(c, s, 6, torch.float64)
        scratch = guarded_scratch(fill) if c.scratch else None
        got = call.run(call.put("pred"), call.put("target"), call.put("var"), c.n, call.put("scale"), tc.HUBER_DELTA,
                       tc.LOOPH_DELTA, call.out.view, None if scratch is None else scratch.view)
        assert scratch is None or scratch.intact(), "a write past the scratch"
        with np.errstate(divide="ignore", invalid="ignore"):
            rel = np.abs(got - ref) / tc.loss_sums_result_relative_bound(c, s)
        print(f"\n[{c.id}] error / ((m + 8) u sum |term|), reported only: " + " ".join(f"{v:.3f}" for v in rel))
        assert_bounded(c, got, ref, bound, f"scratch pre-filled with {fill}")
        runs.append(got)
    if not c.var:
        assert not runs[0][[1, 3, 4, 5]].any(), "var NULL: sums 1, 3, 4, 5 are exactly 0"
    if getattr(c, "equal", False):
        assert not runs[0][[0, 2]].any(), "pred == target: sums 0 and 2 are exactly 0"
    if c.scratch:
        assert runs[0].tobytes() == runs[1].tobytes(), "two calls with scratch (zero / NaN pre-filled) differ in bits"


@pytest.mark.parametrize("c", tc.cases_of("column_sums"), ids=ids(tc.cases_of("column_sums")))
def test_column_sums(c):
    s = tc.make_inputs(c)
    ref, bound = tc.ref_column_sums(c, s)
    runs = []
    for fill in (0.0, float("nan")) if c.scratch else (None,):
        call = Call(c, s, c.R, torch.float64)
        scratch = guarded_scratch(fill) if c.scratch else None
        got = call.run(call.put("x"), c.n, c.R, call.out.view, None if scratch is None else scratch.view)
        assert scratch is None or scratch.intact(), "a write past the scratch"
        assert_bounded(c, got, ref, bound, f"scratch pre-filled with {fill}")
        runs.append(got)
    if c.scratch:
        assert runs[0].tobytes() == runs[1].tobytes(), "two calls with scratch (zero / NaN pre-filled) differ in bits"


@pytest.mark.parametrize("dtype", tc.DTYPES)
def test_column_sums_refuses_more_columns_than_the_scratch_holds(dtype):
    from muygpys_amd import _lib

    c = tc.make_case("column_sums", dtype, R=tc.SCRATCH_DOUBLES + 1, n=1, scratch=True)
    s = tc.make_inputs(c)
    call = Call(c, s, c.R, torch.float64)
    scratch = guarded_scratch(float("nan"))
    call.run(call.put("x"), c.n, c.R, call.out.view, scratch.view, expect=_lib.EUNSUPPORTED)
    assert scratch.untouched()


# ---- prepared table -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", tc.cases_of("table_pack"), ids=ids(tc.cases_of("table_pack")))
def test_table_pack(c):
    from muygpys_amd import _lib

    it = tc.ITEMSIZE[c.dtype]
    assert _lib.load().mgp_packed_row_bytes(c.d, c.R, it) == tc.packed_row_bytes(c.d, c.R, it)
    s = tc.make_inputs(c)
    call = Call(c, s, c.n * c.stride // it)
    got = call.run(call.put("feat"), call.put("targets"), c.n, c.d, c.R, call.out.view, c.stride)
    assert_exact(c, got, tc.ref_table_pack(c, s))


# ---- empty calls ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", tc.DTYPES)
def test_empty_calls_return_ok_and_write_nothing(dtype):
    """b = 0 / n = 0 on every entry: MGP_OK, the output untouched -- but for the two reductions, whose sums of nothing
    are zeros (R = 0 columns: nothing at all)."""
    from muygpys_amd import _lib

    lib, T, st = _lib.load(), TORCH_DTYPE[dtype], _lib.stream_ptr
    x = torch.ones(64, dtype=T, device="cuda")
    idx = torch.zeros(8, dtype=torch.int64, device="cuda")
    p = _lib.ptr
    fn = lambda name: getattr(lib, f"mgp_{name}_{dtype}")
    out = Guarded(16, T)
    calls = {
        "crosswise_diffs": lambda: fn("crosswise_diffs")(p(x), p(x), 4, p(idx), p(idx), 0, 2, p(out.view), st()),
        "crosswise_diffs, batch_idx NULL": lambda: fn("crosswise_diffs")(p(x), p(x), 4, None, p(idx), 0, 2, p(out.view), st()),
        "pairwise_diffs": lambda: fn("pairwise_diffs")(p(x), 4, p(idx), 0, 2, p(out.view), st()),
        "crosswise_dists": lambda: fn("crosswise_dists")(p(x), p(x), 4, p(idx), p(idx), 0, 2, _lib.METRIC_IDS["l2"], p(out.view), st()),
        "pairwise_dists (wave)": lambda: fn("pairwise_dists")(p(x), 4, p(idx), 0, 2, _lib.METRIC_IDS["F2"], p(out.view), st()),
        "pairwise_dists (tile)": lambda: fn("pairwise_dists")(p(x), 4, p(idx), 0, 65, _lib.METRIC_IDS["F2"], p(out.view), st()),
        "reduce_diffs": lambda: fn("reduce_diffs")(p(x), 0, 4, None, _lib.METRIC_IDS["l2"], p(out.view), st()),
        "kernel_apply": lambda: fn("kernel_apply")(p(x), 0, _lib.KERNEL_IDS["matern25"], 1.0, p(out.view), st()),
        "perturb": lambda: fn("perturb")(p(x), 0, 2, _lib.NOISE_SCALAR, 0.1, None, p(out.view), st()),
        "table_pack": lambda: fn("table_pack")(p(x), p(x), 0, 4, 1, p(out.view), 64, st()),
    }
    for name, call in calls.items():
        rc = call()
        torch.cuda.synchronize()
        assert rc == _lib.OK, (name, rc)
        assert out.untouched(), f"{name}: an empty call wrote to its output"
    sums = Guarded(6, torch.float64)
    scratch = guarded_scratch(float("nan"))
    for name, call, zeros in (
        ("loss_sums, scratch", lambda: fn("loss_sums")(p(x), p(x), p(x), 0, None, 1.5, 3.0, p(sums.view), p(scratch.view), st()), 6),
        ("loss_sums", lambda: fn("loss_sums")(p(x), p(x), None, 0, None, 1.5, 3.0, p(sums.view), None, st()), 6),
        ("column_sums, n = 0", lambda: fn("column_sums")(p(x), 0, 3, p(sums.view), p(scratch.view), st()), 3),
        ("column_sums, R = 0", lambda: fn("column_sums")(p(x), 5, 0, p(sums.view), None, st()), 0),
    ):
        sums.view.fill_(float("nan"))
        rc = call()
        torch.cuda.synchronize()
        assert rc == _lib.OK, (name, rc)
        got = sums.numpy()
        assert sums.intact() and scratch.untouched(), name
        assert not got[:zeros].any() and np.isnan(got[zeros:]).all(), (name, got)


def test_zz_report_worst_ratios():
    """Prints the table of the module docstring from this run (python -m pytest -s); asserts nothing new."""
    print("\n    entry             fp32     fp64")
    for entry in tc.ENTRIES:
        r = [RATIOS.get((entry, dt)) for dt in tc.DTYPES]
        if any(v is not None for v in r):
            print(f"    {entry:<17s} " + "    ".join("  -  " if v is None else f"{v:5.3f}" for v in r))
