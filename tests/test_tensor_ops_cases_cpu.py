"""CPU: the case tables of tests/tensor_ops_cases.py reach every launch route of csrc/mgp_tensor_ops.hip and both sides
of every grid cap; its references restate the definitions oracle/muygps_oracle.py restates; and numpy emulations of the
kernels' arithmetic stay inside the bounds the GPU test asserts."""

import collections
import os
import re

import numpy as np
import pytest

from oracle import muygps_oracle as orc
from tests import tensor_ops_cases as tc

SOURCE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "muygpys_amd", "csrc", "mgp_tensor_ops.hip")


def test_case_ids_are_unique_and_every_entry_has_cases():
    ids = [c.id for c in tc.CASES]
    assert len(ids) == len(set(ids))
    assert {c.entry for c in tc.CASES} == set(tc.ENTRIES)
    assert {c.dtype for c in tc.CASES} == set(tc.DTYPES)


@pytest.mark.parametrize("dtype", tc.DTYPES)
@pytest.mark.parametrize("entry", tc.ENTRIES)
def test_every_route_is_reached_at_least_twice(entry, dtype):
    seen = collections.Counter(tc.case_route(c) for c in tc.cases_of(entry) if c.dtype == dtype)
    want = tc.all_routes(entry, tc.ITEMSIZE[dtype])
    assert set(seen) == want, (sorted(want - set(seen)), sorted(set(seen) - want))
    assert min(seen.values()) >= 2, {r: n for r, n in seen.items() if n < 2}


def test_route_count():
    # per dtype: 8 wave instantiations (NP x blocks of 16 features), each in its vec and its scalar form; tile; thread
    assert len(tc.all_routes("pairwise_dists", 4)) == 18 and len(tc.all_routes("pairwise_dists", 8)) == 18
    for dtype in tc.DTYPES:
        waves = {tc.case_route(c) for c in tc.cases_of("pairwise_dists") if c.dtype == dtype} - {"tile", "thread"}
        assert len(waves) == 16


@pytest.mark.parametrize("dtype", tc.DTYPES)
@pytest.mark.parametrize("entry", tc.ENTRIES)
def test_every_route_has_a_case_at_its_grid_cap_and_one_past_it(entry, dtype):
    at, past = set(), set()
    for c in tc.cases_of(entry):
        if c.dtype != dtype:
            continue
        r = tc.case_route(c)
        # the 16 wave variants share one kernel body and one grid rule per NP: counted per NP
        r = re.sub(r"_s\d_(vec|scalar)", "", r)
        items, cap = tc.work_items(c), tc.case_cap(c)
        if items == cap:
            at.add(r)
        if items > cap:
            past.add(r)
    routes = {re.sub(r"_s\d_(vec|scalar)", "", r) for r in tc.all_routes(entry, tc.ITEMSIZE[dtype])}
    assert past == routes, sorted(routes - past)
    assert at, "no case exactly at the cap"


def test_listed_boundaries_are_in_the_tables():
    pd = tc.cases_of("pairwise_dists")
    for dtype in tc.DTYPES:
        mine = [c for c in pd if c.dtype == dtype]
        assert {c.k for c in mine} >= set(tc.PD_K) and {c.d for c in mine} >= set(tc.PD_D)
        for k in tc.PD_K:
            assert {c.b for c in mine if c.k == k} >= {1, 2, 3}
        kmax = {"f32": 157, "f64": 78}[dtype]
        assert {(c.k, c.d) for c in mine} >= {(65, 1), (65, 64), (1, 65), (64, 65), (kmax, 65), (kmax + 1, 65)}
        assert tc.route("pairwise_dists", tc.ITEMSIZE[dtype], 65, kmax, True) == "tile"
        assert tc.route("pairwise_dists", tc.ITEMSIZE[dtype], 65, kmax + 1, True) == "thread"
        assert any(c.d % 2 == 0 for c in mine if tc.case_route(c) == "tile")
        cs = [c for c in tc.cases_of("column_sums") if c.dtype == dtype]
        assert {c.R for c in cs} == {1, 2, 6, 7, 16} and {c.scratch for c in cs} == {True, False}
        ls = [c for c in tc.cases_of("loss_sums") if c.dtype == dtype]
        assert {c.n for c in ls} >= {1, 63, 64, 255, 256, 257, 262145}
        assert {(c.var, c.scale, c.scratch) for c in ls} >= {(v, s, w) for v, s in ((False, False), (True, False), (True, True))
                                                             for w in (True, False)}
        ka = [c for c in tc.cases_of("kernel_apply") if c.dtype == dtype]
        assert {(c.kernel, c.scale) for c in ka} == {(k, s) for k in tc.KERNELS for s in (1.0, 0.37)}
        for entry in ("crosswise_diffs", "pairwise_diffs"):
            names = {c.mis for c in tc.cases_of(entry) if c.dtype == dtype and c.mis}
            assert names == ({("fq",), ("fn",), ("out",)} if entry == "crosswise_diffs" else {("f",), ("out",)})
            assert all(tc.case_route(c) == "scalar" for c in tc.cases_of(entry) if c.mis)
    # the fp32 example of the wave kernels' capacity grid: k = 3, d = 4 strides from b = 8193 on
    assert tc.grid_cap("pairwise_dists", 4, d=4, k=3) == 4096
    assert tc.grid_cap("column_sums", R=7, scratch=True) == 877 * 256 and tc.grid_cap("column_sums", R=6, scratch=True) == 262144
    assert tc.reduce_blocks(1, 6145, True) == 0  # the refused call


def test_constants_restate_the_source():
    with open(SOURCE) as f:
        src = f.read()
    with open(os.path.join(os.path.dirname(SOURCE), "mgp_launch.h")) as f:
        launch = f.read()
    assert "static const int kBlock = 256;" in src and "kAssumedCus * 32" in src
    assert "static const int kReduceBlocks = 1024;" in src and "return kReduceBlocks * 6;" in src
    assert "lds <= 40 * 1024" in src and "Capacity{16}" in src and "Capacity{32}" in src
    assert "kAssumedCus = 256LL" in launch and "kLdsGranule = 1280" in launch and "kCuLdsBytes = 160 * 1024" in launch


def test_largest_case_allocates_under_256_mb():
    worst = max(tc.CASES, key=tc.alloc_bytes)
    assert tc.alloc_bytes(worst) < 256 * 2 ** 20, (worst.id, tc.alloc_bytes(worst))


# ---- the references restate the oracle's definitions ------------------------------------------------------------------------

def _close(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape
    assert np.all(np.abs(a - b) <= 1e-14 * np.maximum(np.abs(a), np.abs(b))), float(np.abs(a - b).max())


@pytest.mark.parametrize("dtype", tc.DTYPES)
def test_tensor_references_agree_with_the_oracle(dtype):
    for c in tc.CASES:
        if c.dtype != dtype or tc.alloc_bytes(c) > 1 << 16:
            continue
        s = tc.make_inputs(c)
        if c.entry == "crosswise_diffs":
            bi = s.bidx if s.bidx is not None else np.arange(c.b)
            assert np.array_equal(tc.ref_crosswise_diffs(s.fq, s.fn, s.bidx, s.nidx), orc.crosswise_tensor(s.fq, s.fn, bi, s.nidx))
        elif c.entry == "pairwise_diffs":
            assert np.array_equal(tc.ref_pairwise_diffs(s.f, s.nidx), orc.pairwise_tensor(s.f, s.nidx))
        elif c.entry == "crosswise_dists":
            bi = s.bidx if s.bidx is not None else np.arange(c.b)
            diffs = orc.crosswise_tensor(s.fq.astype(np.float64), s.fn.astype(np.float64), bi, s.nidx)
            _close(tc.ref_crosswise_dists(c, s)[0], orc.metric_reduce(diffs, c.metric))
        elif c.entry == "pairwise_dists":
            _close(tc.ref_pairwise_dists(c, s)[0], orc.metric_reduce(orc.pairwise_tensor(s.f.astype(np.float64), s.nidx), c.metric))
        elif c.entry == "reduce_diffs":
            x = s.diffs.astype(np.float64)
            want = orc.metric_reduce(x, c.metric) if s.ls is None else orc.anisotropy(x, s.ls.astype(np.float64), c.metric)
            _close(tc.ref_reduce_diffs(c, s)[0], want)
        elif c.entry == "perturb":
            K = s.Kin.astype(np.float64)
            T = tc.NP_DTYPE[dtype]
            want = (orc.homoscedastic_perturb(K, float(T(s.eps))) if c.mode == "scalar"
                    else orc.heteroscedastic_perturb(K, s.noise.astype(np.float64)))
            got = tc.ref_perturb(c, s)
            u = tc.UNIT[dtype]
            assert np.all(np.abs(got - want) <= u * np.abs(want))  # one rounding of the dtype on the diagonal ...
            off = ~np.eye(c.k, dtype=bool)
            assert np.array_equal(got[:, off], s.Kin[:, off])      # ... none off it


@pytest.mark.parametrize("dtype", tc.DTYPES)
def test_kernel_references_agree_with_the_oracle(dtype):
    for c in tc.cases_of("kernel_apply"):
        if c.dtype != dtype or c.n > 257:
            continue
        s = tc.make_inputs(c)
        ref, bound, inside = tc.ref_kernel_apply(c, s)
        x = s.x.astype(np.float64) * float(tc.NP_DTYPE[dtype](c.scale))
        want = orc.KERNELS[c.kernel](x)
        # (the oracle writes x * sqrt(5) and K**2 / 3 in fp64: 1e-14 apart wherever the result is a normal number)
        ok = inside & (want > 1e-290)
        assert ok.sum() >= c.n - 3 - 12
        assert np.all(np.abs(ref[ok].astype(np.float64) - want[ok]) <= (1e-14 + 4 * 2.0 ** -53 * np.asarray(tc.kernel_argument(c.kernel, x)[ok])) * want[ok])
        if c.n > 1:
            assert not inside[-3:].any() and inside[:-3].all(), "the grid ends inside the normal range, three inputs lie beyond"
            assert np.all(ref[-3:] < tc.ref_kernel_end(c)) and np.all(np.isfinite(bound[inside]))


@pytest.mark.parametrize("dtype", tc.DTYPES)
def test_loss_references_agree_with_the_oracle(dtype):
    for c in tc.cases_of("loss_sums"):
        if c.dtype != dtype or c.n > 1000 or not c.var:
            continue
        s = tc.make_inputs(c)
        ref, bound = tc.ref_loss_sums(c, s)
        p, t, v = (a.astype(np.float64) for a in (s.pred, s.target, s.var))
        scale = 1.0 if s.scale is None else float(s.scale[0])
        want = [orc.mse_fn(p, t) * c.n, orc.lool_fn(p, t, v, scale), orc.pseudo_huber_fn(p, t, tc.HUBER_DELTA),
                orc.looph_fn(p, t, v, scale, tc.LOOPH_DELTA)]
        terms, mags = tc.loss_terms(p, t, v, None if s.scale is None else scale)
        for i in range(4):
            # numpy's own fp64 summation of n terms against the exact sum: n roundings of the magnitudes at most
            assert abs(ref[i] - want[i]) <= 1e-14 * abs(want[i]) + (c.n + 8) * 2.0 ** -53 * float(np.sum(mags[i])), (c.id, i)
        if c.n <= 64 and not getattr(c, "equal", False) and not getattr(c, "spread", False):
            _close(ref[[0, 1, 3]], np.array(want)[[0, 1, 3]])
        assert np.all(bound >= 0) and np.all(np.isfinite(bound))


def test_column_sum_reference_is_the_exact_sum():
    c = next(c for c in tc.cases_of("column_sums") if c.n == 257 and c.R == 7 and c.dtype == "f32")
    s = tc.make_inputs(c)
    ref, bound = tc.ref_column_sums(c, s)
    _close(ref, s.x.astype(np.float64).sum(0))
    assert np.all(bound > 0)


def test_table_pack_reference_layout():
    c = next(c for c in tc.cases_of("table_pack") if c.dtype == "f32" and c.d == 5 and c.R == 3 and c.n == 3)
    s = tc.make_inputs(c)
    out = tc.ref_table_pack(c, s)
    assert out.shape == (3, c.stride // 4) and out.tobytes()[: 5 * 4] == s.feat[0].tobytes()
    assert np.array_equal(out[:, 5:8], s.targets) and not out[:, 8:].any()
    assert tc.packed_row_bytes(40, 1, 4) == 192 and tc.packed_row_bytes(1, 0, 8) == 64


# ---- numpy emulations of the kernels' arithmetic stay inside the bounds ----------------------------------------------------

@pytest.mark.parametrize("metric", tc.METRICS)
@pytest.mark.parametrize("d", (1, 3, 16, 65))
def test_sequential_fp32_sum_of_squares_stays_inside_the_distance_bound(d, metric):
    rng = np.random.default_rng(d)
    a, b = rng.standard_normal((2, 4000, d)).astype(np.float32)
    acc = np.zeros(4000, dtype=np.float32)
    for c in range(d):
        df = a[:, c] - b[:, c]
        acc = acc + df * df
    got = np.sqrt(acc) if metric == "l2" else acc
    ref = tc.ref_metric(a.astype(np.float64) - b.astype(np.float64), metric)
    ratio = np.abs(got.astype(np.float64) - ref) / tc.dist_bound(ref, d, metric, "f32")
    print(f"d={d} {metric}: worst error / bound {ratio.max():.3f}")
    assert ratio.max() <= 1.0, ratio.max()


@pytest.mark.parametrize("kernel", tc.KERNELS)
def test_fp32_kernel_formulas_stay_inside_the_kernel_bound(kernel):
    c = next(c for c in tc.cases_of("kernel_apply") if c.dtype == "f32" and c.kernel == kernel and c.n == 257 and c.scale == 0.37)
    s = tc.make_inputs(c)
    ref, bound, inside = tc.ref_kernel_apply(c, s)
    F = np.float32
    x = s.x * F(c.scale)
    if kernel == "rbf":
        got = np.exp(-x * F(0.5))
    elif kernel == "matern05":
        got = np.exp(-x)
    elif kernel == "matern15":
        t = x * F(1.7320508075688772935)
        got = (F(1) + t) * np.exp(-t)
    elif kernel == "matern25":
        t = x * F(2.2360679774997896964)
        got = (F(1) + t + t * t * F(1.0 / 3.0)) * np.exp(-t)
    else:
        got = np.exp(-x * x * F(0.5))
    assert got.dtype == np.float32
    ratio = np.abs(got.astype(np.float64) - ref)[inside] / bound[inside]
    print(f"{kernel}: worst error / bound {ratio.max():.3f}")
    assert ratio.max() <= 1.0, ratio.max()


def test_fp64_reduction_emulation_stays_inside_the_reduction_bound():
    c = next(c for c in tc.cases_of("loss_sums") if c.dtype == "f32" and c.n == 257 and c.var and c.scale and c.scratch
             and not getattr(c, "equal", False))
    s = tc.make_inputs(c)
    ref, bound = tc.ref_loss_sums(c, s)
    terms, _ = tc.loss_terms(s.pred.astype(np.float64), s.target.astype(np.float64), s.var.astype(np.float64), float(s.scale[0]))
    got = np.array([np.cumsum(t)[-1] for t in terms])  # a plain sequential fp64 sum: a longer path than the kernel's
    assert np.all(np.abs(got - ref) <= bound * (257 + 8) / (tc.reduce_path_adds(257, 2, True) + 8))
