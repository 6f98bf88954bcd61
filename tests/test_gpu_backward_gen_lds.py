"""GPU: the vector-Jacobian product of the general-smoothness Matern in LDS (csrc/mgp_backward_gen.hip:
``mgp_posterior_backward_gen_*``) -- every one of its six outputs against the fp64 reference of
tests/gen_vjp_reference.py / tests/gen_backward_reference.py (pinned to central differences on the CPU) at the edges
of the built kernel, against the closed-form entries at nu = 1/2, 3/2, 5/2 and against the slab entry (no oracle
involved), placement invariance of the hyper-parameter partials bit for bit, failure semantics and zero distances, the
``fused.gen_backward`` switch and ``autograd.posterior``.  Every check asserts the kernel that served it by name.

Edges of the built kernel.  Threads: 64 up to k + 2 = 64 rows, 128 up to 128 rows, 256 beyond.  A strip of the
covariance and of the pair-cotangent phase is NT threads x 4 pairs in fp32, x 2 in fp64; with 64 threads that is 256
pairs in fp32 (k = 22 has 253, k = 23 has 276) and 128 in fp64 (k = 15: 120, k = 16: 136).  k = 62 | 63: the last
single-wave factorisation and the first ``factor_augmented_lds`` (128 threads); k = 126 | 127: 128 | 256 threads
(fp32 alone: the fp64 limit lies below); the limit of ``mgp_max_nn_count_backward_gen`` and the k before it in either
width.  d = 70 gives two feature chunks (64 + 6) wherever 64 features fit LDS next to the system, per-feature scales
across them.

Inputs and bands as tests/test_gpu_gen_backward.py: the length scale grows with sqrt(d / 8), F2 goes with nu <= 1/2
beyond two points; fp64 1e-5, fp32 3e-3 through ``assert_close`` (|err| <= rtol |ref| + rtol rms(ref)), fp32 grad_nu
asserted up to nu = 4 and finite above.  The accumulated tables are compared on the rows a neighbourhood reads (the rms
is theirs); every other row must still hold what it held.

The fp32 cases of the edge sample were fixed after pushing the float32 restatement of covariances
(tests/test_matern_gen_cpu.py) and derivatives (tests/gen_deriv_restatement.py) through the fp64 reference on each
case's own inputs on the CPU: the sample keeps the cases on which that deviation stays below a tenth of the band for
every output (FP32_EXCLUDED lists the combinations that did not, with the figure)."""

import numpy as np
import pytest
import torch

from tests import gen_vjp_reference as VR
from tests.test_gpu_gen_backward import NU32_LIMIT, scales
from tests.test_gpu_gen_backward import entry as slab_entry
from tests.test_gpu_large_backward import (GRAD_RTOL, LS, NUGGET, TORCH, _functor_problem, cotangents, length_scales,
                                           make_table, neighbourhoods)
from tests.util import assert_close, to_dev

pytestmark = pytest.mark.gpu

ALL = ("fq", "fn", "tg", "ls", "noise", "nu")
METRIC = {"l2": 0, "F2": 1}


def limit(dtype):
    from muygpys_amd import _lib

    return int(_lib.load().mgp_max_nn_count_backward_gen(4 if dtype == "float32" else 8))


def kernel_name(dtype, nu_output):
    return f"mgp::backward_gen_kernel<{'float' if dtype == 'float32' else 'double'}, {'true' if nu_output else 'false'}>"


def entry(dtype, Xq_d, Xn_d, bi_d, ni_d, Y_d, noise, nu, metric, ls, gm, gv, gyk, want=ALL, sentinel=0.0):
    """One ``mgp_posterior_backward_gen_*`` call.  ``noise``: a float, a (n,) table or a (b, k) tensor on the device.
    Returns ({name: tensor pre-filled with ``sentinel``, or None where not asked for}, info)."""
    from muygpys_amd import _lib

    t = TORCH[dtype]
    P = _lib.ptr
    b, k = ni_d.shape
    d, R = Xn_d.shape[1], Y_d.shape[1]
    ls_d = to_dev(np.atleast_1d(ls), t)
    mode = (0, noise, None) if isinstance(noise, float) else (1 if noise.ndim == 1 else 2, 0.0, P(noise))
    shapes = dict(fq=tuple(Xq_d.shape), fn=tuple(Xn_d.shape), tg=tuple(Y_d.shape), ls=(b, ls_d.numel()), noise=(b, k), nu=(b,))
    out = {n: torch.full(shapes[n], sentinel, device="cuda", dtype=t) if n in want else None for n in ALL}
    info = torch.zeros(1, dtype=torch.int32, device="cuda")
    cot = [None if g is None else to_dev(g, t) for g in (gm, gv, gyk)]
    rc = _lib.fn("posterior_backward_gen", t)(P(Xq_d), P(Xn_d), d, P(bi_d), P(ni_d), b, k, P(Y_d), R, *mode, float(nu),
                                              METRIC[metric], P(ls_d), ls_d.numel(), *[P(g) for g in cot],
                                              *[P(out[n]) for n in ALL], P(info), _lib.stream_ptr())
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert _lib.last_kernel().startswith(kernel_name(dtype, "nu" in want) + " [threads="), _lib.last_kernel()
    threads = 64 if k + 2 <= 64 else (128 if k + 2 <= 128 else 256)
    assert f"[threads={threads}," in _lib.last_kernel(), _lib.last_kernel()
    return out, int(info.item())


def reference(Xq, Xn, bi, ni, Y, rows, nu, metric, ls, gm, gv, gyk, want=ALL, **pieces):
    """{name: fp64 array} of the outputs in ``want``."""
    ref = {}
    if set(want) & {"ls", "noise", "nu"}:
        hyper = {k_: v for k_, v in pieces.items() if k_ in ("kernel_fn", "dk_dr", "dk_dnu")}
        ref["ls"], ref["noise"], ref["nu"] = VR.partials(Xq, Xn, bi, ni, Y, rows, nu, metric, ls, gm, gv, gyk, **hyper)
    if set(want) & {"fq", "fn", "tg"}:
        feat = {k_: v for k_, v in pieces.items() if k_ in ("kernel_fn", "dk_dr")}
        ref["fq"], ref["fn"], ref["tg"] = VR.vjp(Xq, Xn, bi, ni, Y, rows, nu, metric, ls, gm, gv, gyk, **feat)
    return {n: ref[n] for n in want}


def touched_rows(name, bi, ni):
    return np.unique(bi) if name == "fq" else np.unique(ni)


def check(got, ref, dtype, nu, bi, ni, what, sentinel=0.0):
    """Every output in ``ref`` inside the band; rows of the accumulated tables that no neighbourhood (``bi``, ``ni``)
    reads still at the sentinel."""
    for name, r in ref.items():
        g = got[name].double().cpu().numpy()
        if name in ("fq", "fn", "tg"):
            rows = touched_rows(name, bi, ni)
            rest = np.setdiff1d(np.arange(len(g)), rows)
            assert (g[rest] == sentinel).all(), (what, name, "a row nobody reads was written")
            g, r = g[rows] - sentinel, r[rows]
        print(f"{what}: {name} max |err| {np.abs(g - r).max():.3e}, rms(ref) {np.sqrt(np.mean(r * r)):.3e}")
        assert np.isfinite(g).all(), (what, name)
        if name == "nu" and dtype == "float32" and nu > NU32_LIMIT:
            continue  # (the fp32 evaluator's dk/dnu error is a large fraction of the derivative: tests/test_gpu_gen_backward.py)
        assert_close(g, r, GRAD_RTOL[dtype], f"{what}: {name}")


# ---- 1. the entry against the reference: a spread sample over every axis -------------------------------------------------
def edge_ks(dtype):
    lim = limit(dtype)
    strip = (22, 23) if dtype == "float32" else (15, 16)
    return tuple(k for k in (1, 2, *strip, 62, 63, 126, 127, lim - 1, lim) if k <= lim)


EDGE_D = (1, 3, 8, 70)
EDGE_NU = (0.3, 0.42, 1.0, 2.2, 3.7, 8.0)
FORMS = ("loocv", "posterior", "posterior3")
# every non-empty pattern of the six outputs appears: the 63 subsets are dealt over the cases, two per case and more
WANT_PATTERNS = tuple(tuple(n for i, n in enumerate(ALL) if (m >> i) & 1) for m in range(1, 64))
# fp32 combinations taken out of the sample by the CPU measurement of the module docstring, as (what matches, what it
# becomes): one feature under F2 -- the scaled squared distances of neighbours on a line reach the evaluators' lower
# clamp on x (the case that needed a band of its own in tests/test_gpu_gen_backward.py; here 11.4 bands on grad_feat_nn
# at k = 62, nu = 0.42) -- goes to l2; sixty-three points on a line (k = 62, d = 1: 0.19 of the band on grad_noise under
# l2 as well) get three features; grad_nu at (k = 62, d = 8, nu = 3.7), 0.18 of the band, goes to nu = 2.2
FP32_EXCLUDED = ((dict(d=1, metric="F2"), dict(metric="l2")), (dict(k=62, d=1), dict(d=3)),
                 (dict(k=62, d=8, nu=3.7), dict(nu=2.2)))


def _fp32_excluded(c):
    return [to for match, to in FP32_EXCLUDED if c["dtype"] == "float32" and all(c[n] == v for n, v in match.items())]


def _edge_cases():
    rng = np.random.default_rng(20261022)
    n_cases = 40

    def spread(values):
        reps = -(-n_cases // len(values))
        return [values[i] for i in rng.permutation(np.tile(np.arange(len(values)), reps))[:n_cases]]

    cols = dict(dtype=spread(("float32", "float64")), d=spread(EDGE_D), nu=spread(EDGE_NU), metric=spread(("l2", "F2")),
                aniso=spread((False, True)), noise=spread(("scalar", "table", "batch")), bi=spread((True, False)),
                shared=spread((False, True)), form=spread(FORMS))
    cases = [{name: vals[i] for name, vals in cols.items()} for i in range(n_cases)]
    # the k edges of a width are dealt over its cases in turn (twenty cases a width: every edge at least once)
    turn = {"float32": 0, "float64": 0}
    for c in cases:
        ks = edge_ks(c["dtype"])
        c["k"] = ks[turn[c["dtype"]] % len(ks)]
        turn[c["dtype"]] += 1
    # ... and the combinations at which the kernel takes a path of its own: k edges with per-feature scales in the width
    # they belong to; two feature chunks at the limit and next to the thread switch in both widths; nu below 1/2
    forced = [(dt, k, 8 if j % 2 else 3, EDGE_NU[j % len(EDGE_NU)]) for dt in ("float32", "float64")
              for j, k in enumerate(edge_ks(dt)) if k > 2][::2]
    forced += [("float32", limit("float32"), 70, 0.42), ("float64", limit("float64"), 70, 2.2), ("float32", 63, 70, 1.0),
               ("float64", 62, 70, 0.3)]
    for j, (dtype, k, d, nu) in enumerate(forced):
        base = dict(cases[j])
        base.update(k=k, d=d, dtype=dtype, nu=nu, aniso=True)
        cases.append(base)
    low = 0
    for c in cases:
        for to in _fp32_excluded(c):
            c.update(to)
        # F2 with more than two points: nu <= 1/2 (tests/test_gpu_gen_backward.py)
        if c["metric"] == "F2" and c["k"] > 2 and c["nu"] > 0.5:
            c["nu"] = (0.3, 0.42)[low % 2]
            low += 1
    # the first sixteen cases ask for all six outputs; the others for one subset each; the subsets that are left ride
    # along as second calls on the same inputs
    for i, c in enumerate(cases):
        c["want"] = WANT_PATTERNS[(i * 37) % 63] if i >= 16 else ALL
    used = {c["want"] for c in cases}
    rest = [w for w in WANT_PATTERNS if w not in used]
    for i, c in enumerate(cases):
        c["also"] = tuple(rest[i::len(cases)])
    return cases


EDGE_CASES = _edge_cases()


def _edge_id(c):
    return (f"k{c['k']}-d{c['d']}-nu{c['nu']}-{c['metric']}-{'aniso' if c['aniso'] else 'iso'}-{c['noise']}"
            f"-{'bi' if c['bi'] else 'nobi'}-{'one' if c['shared'] else 'two'}-{c['form']}-{'+'.join(c['want'])}-{c['dtype']}")


def test_edge_sample_covers_every_factor():
    for dtype in ("float32", "float64"):
        assert {c["k"] for c in EDGE_CASES if c["dtype"] == dtype} >= set(edge_ks(dtype)), dtype
    seen = {name: {c[name] for c in EDGE_CASES} for name in EDGE_CASES[0] if name != "also"}
    assert seen["d"] == set(EDGE_D) and seen["nu"] == set(EDGE_NU)
    assert seen["metric"] == {"l2", "F2"} and seen["noise"] == {"scalar", "table", "batch"}
    assert seen["aniso"] == {False, True} and seen["bi"] == {False, True} and seen["form"] == set(FORMS)
    assert seen["shared"] == {False, True} and seen["dtype"] == {"float32", "float64"}
    patterns = seen["want"] | {w for c in EDGE_CASES for w in c["also"]}
    assert patterns == set(WANT_PATTERNS) and len(WANT_PATTERNS) == 63
    assert len(EDGE_CASES) <= 60
    assert not any(_fp32_excluded(c) for c in EDGE_CASES)
    # the limits the docstring's edges assume
    assert limit("float32") >= 127 > limit("float64") >= 63
    from muygpys_amd import _lib

    assert _lib.METRIC_IDS == METRIC


def edge_problem(c):
    """The inputs of one edge case, on the host."""
    rng = np.random.default_rng(sum(map(ord, _edge_id(c))))
    k, d, b, n = c["k"], c["d"], 5, 300
    gm, gv, gyk, R = cotangents(rng, c["form"], b)
    Xn, Y = make_table(rng, n, d, R)
    Xq = Xn if c["shared"] else rng.uniform(size=(40, d))
    ni = neighbourhoods(rng, n, b, k)
    bi = rng.choice(len(Xq), size=b, replace=False) if c["bi"] else np.arange(b)
    ls = scales(rng, d, c["aniso"])
    table = NUGGET * (1.0 + rng.uniform(size=n))
    rows = np.full((b, k), NUGGET) if c["noise"] == "scalar" else table[ni]
    return Xq, Xn, Y, bi, ni, ls, table, rows, (gm, gv, gyk)


@pytest.mark.parametrize("c", EDGE_CASES, ids=[_edge_id(c) for c in EDGE_CASES])
def test_kernel_edges_against_the_reference(c):
    dtype, nu = c["dtype"], c["nu"]
    Xq, Xn, Y, bi, ni, ls, table, rows, cot = edge_problem(c)
    t = TORCH[dtype]
    noise = NUGGET if c["noise"] == "scalar" else to_dev(table if c["noise"] == "table" else rows, t)
    Xn_d = to_dev(Xn, t)
    Xq_d = Xn_d if c["shared"] else to_dev(Xq, t)
    full = reference(Xq, Xn, bi, ni, Y, rows, nu, c["metric"], ls, *cot)
    for want in (c["want"], *c["also"]):
        got, info = entry(dtype, Xq_d, Xn_d, to_dev(bi) if c["bi"] else None, to_dev(ni), to_dev(Y, t), noise, nu,
                          c["metric"], ls, *cot, want=want, sentinel=0.25)
        assert info == 0
        assert [got[n] is None for n in ALL] == [n not in want for n in ALL]
        check(got, {n: full[n] for n in want}, dtype, nu, bi, ni, _edge_id(c) + " / " + "+".join(want), sentinel=0.25)


# ---- 2. agreement with the closed forms: no oracle involved ------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("nu, kernel", [(0.5, "matern05"), (1.5, "matern15"), (2.5, "matern25")])
@pytest.mark.parametrize("aniso", [False, True], ids=["iso", "aniso"])
@pytest.mark.parametrize("k, form", [(30, "posterior3"), (70, "posterior"), (30, "loocv"), (70, "loocv")])
def test_agrees_with_the_closed_form_entries(k, form, aniso, nu, kernel, dtype):
    from muygpys_amd import _lib

    rng = np.random.default_rng(int(10 * nu) + aniso + k)
    n, d, b = 400, 8, 8
    gm, gv, gyk, R = cotangents(rng, form, b)
    X, Y = make_table(rng, n, d, R)
    Xq = rng.uniform(size=(30, d))
    ni, bi = neighbourhoods(rng, n, b, k), rng.choice(30, size=b, replace=False)
    ls = length_scales(rng, d, aniso)
    t, P = TORCH[dtype], _lib.ptr
    Xn_d, Y_d, ni_d = to_dev(X, t), to_dev(Y, t), to_dev(ni)
    ls_d = to_dev(np.atleast_1d(ls), t)
    cot = [None if g is None else to_dev(g, t) for g in (gm, gv, gyk)]
    info = torch.zeros(1, dtype=torch.int32, device="cuda")
    kid = _lib.KERNEL_IDS[kernel]
    if form == "loocv":  # (one table on both sides, hyper-parameters alone: what mgp_loocv_backward_* has)
        Xq_d, bi_d, want = Xn_d, to_dev(rng.choice(n, size=b, replace=False)), ("ls", "noise")
        ref = {n_: torch.zeros(s, device="cuda", dtype=t) for n_, s in (("ls", (b, ls_d.numel())), ("noise", (b, k)))}
        rc = _lib.fn("loocv_backward", t)(P(Xn_d), d, P(bi_d), P(ni_d), b, k, P(Y_d), 0, NUGGET, None, kid, 0, P(ls_d),
                                          ls_d.numel(), *[P(g) for g in cot], P(ref["ls"]), P(ref["noise"]), P(info),
                                          _lib.stream_ptr())
    else:
        Xq_d, bi_d, want = to_dev(Xq, t), to_dev(bi), ("fq", "fn", "tg", "ls", "noise")
        shapes = dict(fq=Xq_d.shape, fn=Xn_d.shape, tg=Y_d.shape, ls=(b, ls_d.numel()), noise=(b, k))
        ref = {n_: torch.zeros(tuple(shapes[n_]), device="cuda", dtype=t) for n_ in want}
        rc = _lib.fn("posterior_backward", t)(P(Xq_d), P(Xn_d), d, P(bi_d), P(ni_d), b, k, P(Y_d), R, 0, NUGGET, None, kid, 0,
                                              P(ls_d), ls_d.numel(), P(cot[0]), P(cot[1]), *[P(ref[n_]) for n_ in want],
                                              P(info), _lib.stream_ptr())
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert int(info.item()) == 0
    got, bad = entry(dtype, Xq_d, Xn_d, bi_d, ni_d, Y_d, NUGGET, nu, "l2", ls, gm, gv, gyk, want=want)
    assert bad == 0
    for name in want:
        r, g = ref[name].double().cpu().numpy(), got[name].double().cpu().numpy()
        print(f"nu = {nu} vs {kernel}, {form}, k = {k}: {name} max |err| {np.abs(g - r).max():.3e}, rms {np.sqrt(np.mean(r * r)):.3e}")
        assert_close(g, r, GRAD_RTOL[dtype], f"nu = {nu} vs {kernel}: {name}")


# ---- 3. agreement with the slab entry ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("k", [30, "limit"])
@pytest.mark.parametrize("aniso", [False, True], ids=["iso", "aniso"])
def test_agrees_with_the_slab_entry(aniso, k, dtype):
    k = limit(dtype) if k == "limit" else k
    rng = np.random.default_rng(40 + k + aniso)
    n, d, b = 400, 8, 7
    X, Y = make_table(rng, n, d)
    ni, bi = neighbourhoods(rng, n, b, k), rng.choice(n, size=b, replace=False)
    ls = length_scales(rng, d, aniso)
    gm, gv, gyk, _ = cotangents(rng, "loocv", b)
    t = TORCH[dtype]
    X_d = to_dev(X, t)
    args = (to_dev(bi), to_dev(ni), to_dev(Y, t), NUGGET, 1.3, "l2", ls, gm, gv, gyk)
    s_l, s_n, s_nu, bad = slab_entry(dtype, X_d, *args)
    got, info = entry(dtype, X_d, X_d, *args, want=("ls", "noise", "nu"))
    assert bad == 0 and info == 0
    for name, r in (("ls", s_l), ("noise", s_n), ("nu", s_nu)):
        assert_close(got[name].double().cpu().numpy(), r.double().cpu().numpy(), GRAD_RTOL[dtype], f"k = {k}: {name} against the slab")


# ---- 4. placement invariance, bitwise ------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("k", [40, 100], ids=["k40-64-threads", "k100-128-or-256-threads"])
@pytest.mark.parametrize("aniso", [False, True], ids=["iso", "aniso"])
def test_placement_invariance_bitwise(aniso, k, dtype):
    """grad_ls, grad_noise and grad_nu of a neighbourhood: alone, first and last of nine, and in a batch larger than the
    grid (4096 workgroups at most) -- the same bits, over sentinel-filled outputs."""
    from muygpys_amd import _lib

    k = min(k, limit(dtype))
    rng = np.random.default_rng(300 + k)
    n, d, b = 600, 8, 9
    X, Y = make_table(rng, n, d)
    ni, bi = neighbourhoods(rng, n, b, k), rng.choice(n, size=b, replace=False)
    ls = length_scales(rng, d, aniso)
    gm, gv, gyk, _ = cotangents(rng, "loocv", b)
    t = TORCH[dtype]
    Xd, Yd = to_dev(X, t), to_dev(Y, t)

    def run(rows):
        rows = np.asarray(rows)
        got, info = entry(dtype, Xd, Xd, to_dev(bi[rows]), to_dev(ni[rows]), Yd, NUGGET, 1.3, "l2", ls, gm[rows], gv[rows],
                          gyk[rows], want=("ls", "noise", "nu"), sentinel=-777.0)
        assert info == 0
        grid, _ = _lib.last_launch_geometry()
        return {n_: g.cpu().numpy() for n_, g in got.items() if g is not None}, grid

    alone, _ = run([0])
    assert all(np.isfinite(a).all() and (a != -777.0).all() for a in alone.values())
    big = np.concatenate([np.tile(np.arange(1, 9), 640), [0], np.tile(np.arange(1, 9), 3)])  # 5145 neighbourhoods
    for name, rows, pos in (("first of 9", [0, 1, 2, 3, 4, 5, 6, 7, 8], 0), ("last of 9", [1, 2, 3, 4, 5, 6, 7, 8, 0], 8),
                            ("beyond the grid", big, 5120)):
        got, grid = run(rows)
        if name == "beyond the grid":
            assert grid < len(rows), (grid, len(rows))
        for what in ("ls", "noise", "nu"):
            assert alone[what][0].tobytes() == got[what][pos].tobytes(), (name, what, alone[what][0], got[what][pos])


# ---- 5. failure semantics, zero distances ------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("k", [20, 90])
def test_singular_neighbourhoods_are_counted_and_left_untouched(k, dtype):
    rng = np.random.default_rng(6 + k)
    n, nq, d, b = 500, 40, 8, 8
    Xn, Y = make_table(rng, n, d)
    Xq = rng.uniform(size=(nq, d))
    broken = np.array([2, 7])
    good = np.setdiff1d(np.arange(b), broken)
    # the broken neighbourhoods read rows no good one shares
    perm = rng.permutation(n)
    ni = np.stack([rng.choice(perm[:n - 2 * k], size=k, replace=False) for _ in range(b)])
    ni[broken[0]], ni[broken[1]] = perm[n - 2 * k:n - k], perm[n - k:]
    bi = rng.choice(nq, size=b, replace=False)
    ni[broken, 1] = ni[broken, 0]  # a duplicated neighbour ...
    noise = np.full((b, k), NUGGET)
    noise[broken] = 0.0            # ... and no nugget: exactly singular
    gm, gv, gyk, _ = cotangents(rng, "loocv", b)
    ref = reference(Xq, Xn, bi[good], ni[good], Y, noise[good], 1.3, "l2", LS, gm[good], gv[good], gyk[good])
    t, sentinel = TORCH[dtype], -777.0
    got, info = entry(dtype, to_dev(Xq, t), to_dev(Xn, t), to_dev(bi), to_dev(ni), to_dev(Y, t), to_dev(noise, t), 1.3, "l2", LS,
                      gm, gv, gyk, sentinel=sentinel)
    assert info == 2
    for name in ("ls", "noise", "nu"):
        assert (got[name][to_dev(broken)] == sentinel).all(), name
    for name, rows in (("fq", bi[broken]), ("fn", np.unique(ni[broken])), ("tg", np.unique(ni[broken]))):
        assert (got[name][to_dev(rows)] == sentinel).all(), name
    # (check() also finds every row outside the good neighbourhoods at the sentinel)
    check({n_: (g if n_ in ("fq", "fn", "tg") else g[to_dev(good)]) for n_, g in got.items()}, ref, dtype, 1.3, bi[good], ni[good],
          "the six good neighbourhoods", sentinel=sentinel)


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("metric, aniso, nu", [("l2", False, 0.3), ("l2", True, 1.0), ("F2", True, 0.42), ("l2", True, 0.3)])
def test_duplicate_rows_give_finite_values_that_match_the_reference(metric, aniso, nu, dtype):
    """Pairs at zero distance (a neighbour twice, and the query among its neighbours) with a nugget: nothing of them
    reaches a feature, length-scale or smoothness cotangent, below nu = 1/2 -- where dk/dr diverges at 0 -- as elsewhere."""
    rng = np.random.default_rng(8)
    n, d, k, b = 300, 3, 40, 6
    X, Y = make_table(rng, n, d)
    ni, bi = neighbourhoods(rng, n, b, k), rng.choice(n, size=b, replace=False)
    ni[:, 1] = ni[:, 0]
    ni[::2, 5] = bi[::2]
    ls = length_scales(rng, d, aniso)
    gm, gv, gyk, _ = cotangents(rng, "loocv", b)
    rows = np.full((b, k), NUGGET)
    ref = reference(X, X, bi, ni, Y, rows, nu, metric, ls, gm, gv, gyk)
    t = TORCH[dtype]
    X_d = to_dev(X, t)
    got, info = entry(dtype, X_d, X_d, to_dev(bi), to_dev(ni), to_dev(Y, t), NUGGET, nu, metric, ls, gm, gv, gyk)
    assert info == 0
    check(got, ref, dtype, nu, bi, ni, f"duplicates, {metric}, nu = {nu}")


# ---- 6. the fused switch -----------------------------------------------------------------------------------------------------
def _loocv_args(k, seed=31, b=48, n=800, d=4, t=torch.float64):
    X, y, bi, ni = _functor_problem(seed + k, n, b, k, d, np.full(d, 1.2))
    return to_dev(X, t), to_dev(y, t), to_dev(bi), to_dev(ni)


def test_the_default_mode_is_the_slab_and_the_switch_selects_the_lds_kernel():
    from muygpys_amd import _lib, fused

    args = _loocv_args(30)
    spec = lambda ls=1.4, noise=1e-2, nu=1.3: fused.KernelSpec("matern_gen", "l2", ls, noise, smoothness=nu)  # noqa: E731
    assert fused.gen_backward_default() == "slab"
    slab = fused.loocv_value_and_grad(spec(), *args, grad_smoothness=True)
    assert _lib.last_kernel() == "mgp::hyper_backward_gen_large_kernel<double, true>"
    with fused.gen_backward("lds"):
        assert fused.gen_backward_default() == "lds"
        lds = fused.loocv_value_and_grad(spec(), *args, grad_smoothness=True)
        assert _lib.last_kernel().startswith(kernel_name("float64", True)), _lib.last_kernel()
        three = fused.loocv_value_and_grad(spec(), *args)
        assert _lib.last_kernel().startswith(kernel_name("float64", False)), _lib.last_kernel()
        assert len(three) == 3

        def f(**kw):
            return fused.loocv_value_and_grad(spec(**kw), *args)[0]

        fd = np.array([(f(ls=1.4 + 1e-5) - f(ls=1.4 - 1e-5)) / 2e-5, (f(noise=1e-2 + 1e-5) - f(noise=1e-2 - 1e-5)) / 2e-5,
                       (f(nu=1.3 + 1e-5) - f(nu=1.3 - 1e-5)) / 2e-5])
    assert fused.gen_backward_default() == "slab"
    flat = lambda r: np.array([float(np.asarray(r[1]).reshape(-1)[0]), float(r[2]), float(r[3])])  # noqa: E731
    print(f"lds {flat(lds)!r}, slab {flat(slab)!r}, central differences {fd!r}")
    assert lds[0] == slab[0]
    np.testing.assert_allclose(flat(lds), flat(slab), rtol=1e-9)
    np.testing.assert_allclose(flat(lds), fd, rtol=2e-6, atol=2e-7 * np.abs(fd).max())
    with pytest.raises(ValueError, match="gen_backward"):
        with fused.gen_backward("wave"):
            pass


@pytest.mark.parametrize("dtype, k", [("float64", "limit+1"), ("float32", "measured+1")])
def test_beyond_the_lds_limit_the_switch_falls_to_the_slab(dtype, k):
    """... beyond the kernel's limit through the ladder (fp64), beyond the last nn_count at which the rung was measured
    to win (``fused.GEN_BACKWARD_LDS_MAX_NN_COUNT``; fp32: 64, which the LDS kernel itself would serve) without a call."""
    from muygpys_amd import _lib, fused

    k = limit(dtype) + 1 if k == "limit+1" else fused.GEN_BACKWARD_LDS_MAX_NN_COUNT[4 if dtype == "float32" else 8] + 1
    assert k <= limit(dtype) or dtype == "float64"
    args = _loocv_args(k, b=8, n=600, t=TORCH[dtype])
    with fused.gen_backward("lds"):
        got = fused.loocv_value_and_grad(fused.KernelSpec("matern_gen", "l2", 1.4, 1e-2, smoothness=1.3), *args, grad_smoothness=True)
        assert _lib.last_kernel() == f"mgp::hyper_backward_gen_large_kernel<{'float' if dtype == 'float32' else 'double'}, true>"
    assert all(np.isfinite(np.asarray(g, dtype=np.float64)).all() for g in got)


def test_lbfgsb_with_a_free_smoothness_ends_at_the_same_optimum_under_both_modes():
    from muygpys_amd import fused
    from muygpys_amd.optimize import L_BFGS_B_optimize
    from tests.test_gpu_gen_backward import _gen_model

    k, d = 30, 3
    X, y, bi, ni = _functor_problem(4, 2000, 150, k, d, np.full(d, 1.1))
    Xd, yd = to_dev(X, torch.float64), to_dev(y, torch.float64)
    ends = {}
    for mode in ("slab", "lds"):
        m = _gen_model(1.0, 2.0, noise=1e-3)
        cross, pair, y_b, y_nn = m.make_train_tensors(to_dev(bi), to_dev(ni), Xd, yd)
        with fused.gen_backward(mode):
            new = L_BFGS_B_optimize(m, y_b, y_nn, cross, pair, analytic_gradient=True)
        ends[mode] = (float(new.kernel.deformation.length_scale()), float(new.kernel.smoothness()))
    print(f"(length scale, nu): {ends!r}")
    np.testing.assert_allclose(ends["lds"], ends["slab"], rtol=1e-4)


# ---- 7. autograd.posterior ---------------------------------------------------------------------------------------------------
def _autograd_problem(k, shared, seed=5):
    rng = np.random.default_rng(seed + k)
    n, nq, d, b, R = 200, 30, 4, 6, 2
    Xn, Y = make_table(rng, n, d, R)
    Xq = Xn if shared else rng.uniform(size=(nq, d))
    ni = neighbourhoods(rng, n, b, k)
    bi = rng.choice(len(Xq), size=b, replace=False)
    return Xq, Xn, Y, bi, ni, rng.normal(size=(b, R)), rng.normal(size=b)


def _autograd_run(dtype, Xq, Xn, Y, bi, ni, gm, gv, ls, noise, nu, shared, nu_tensor=True):
    from muygpys_amd import _lib, autograd, fused

    t = TORCH[dtype]
    leaf = lambda v: to_dev(np.asarray(v, dtype=np.float64), t).requires_grad_(True)  # noqa: E731
    Xn_d = leaf(Xn)
    Xq_d = Xn_d if shared else leaf(Xq)
    scalar = lambda v: torch.tensor(float(v), device="cuda", dtype=t, requires_grad=True)  # noqa: E731  (0-d)
    Y_d, ls_d, nz_d = leaf(Y), scalar(ls), scalar(noise)
    nu_d = torch.tensor(nu, dtype=torch.float64, requires_grad=True) if nu_tensor else nu
    mean, var = autograd.posterior(fused.KernelSpec("matern_gen", "l2", ls_d, nz_d, smoothness=nu_d), Xq_d, Xn_d, to_dev(bi),
                                   to_dev(ni), Y_d)
    # (the library remembers the last kernel per thread, and the backward runs on the autograd engine's: asked there)
    served = []
    Y_d.register_hook(lambda g: served.append(_lib.last_kernel()))
    ((mean * to_dev(gm, t)).sum() + (var * to_dev(gv, t)).sum()).backward()
    grads = dict(Xq=Xq_d.grad, Xn=Xn_d.grad, Y=Y_d.grad, ls=ls_d.grad, noise=nz_d.grad, nu=nu_d.grad if nu_tensor else None)
    assert len(served) == 1 and served[0].startswith(kernel_name(dtype, nu_tensor) + " [threads="), served
    return mean, var, {n_: None if g is None else g.double().cpu().numpy() for n_, g in grads.items()}


@pytest.mark.parametrize("shared", [False, True], ids=["two-tables", "one-table"])
@pytest.mark.parametrize("k", [12, 40])
def test_autograd_posterior_is_the_central_difference_of_the_reference(k, shared):
    """fp64: d / d (length scale, noise, nu) and a handful of feature and response entries of
    (mean . gm).sum() + (var . gv).sum() against central differences of the fp64 REFERENCE outputs (no GPU
    self-comparison), rtol 2e-6, atol 2e-7 max |fd|; the fp32 run finite and within GRAD_RTOL of the fp64 one."""
    Xq, Xn, Y, bi, ni, gm, gv = _autograd_problem(k, shared)
    ls, noise, nu = 0.6, NUGGET, 1.3
    mean, var, g64 = _autograd_run("float64", Xq, Xn, Y, bi, ni, gm, gv, ls, noise, nu, shared)
    b = len(bi)

    def value(Xq_=None, Xn_=None, Y_=None, ls_=ls, noise_=noise, nu_=nu):
        Xn_ = Xn if Xn_ is None else Xn_
        Xq_ = (Xn_ if shared else Xq) if Xq_ is None else Xq_
        m, v, _ = VR.outputs(Xq_, Xn_, bi, ni, Y if Y_ is None else Y_, np.full((b, k), noise_), nu_, "l2", ls_)
        return (gm * m).sum() + (gv * v).sum()

    m_ref, v_ref, _ = VR.outputs(Xq, Xn, bi, ni, Y, np.full((b, k), noise), nu, "l2", ls)
    assert_close(mean.detach().double().cpu().numpy(), m_ref, 1e-5, "mean")
    assert_close(var.detach().double().cpu().numpy(), v_ref, 1e-5, "var")

    def shifted(A, r, c, s):
        A = A.copy()
        A[r, c] += s
        return A

    h = 1e-6
    pairs = [("ls", g64["ls"].reshape(()), (value(ls_=ls + 1e-5) - value(ls_=ls - 1e-5)) / 2e-5),
             ("noise", g64["noise"].reshape(()), (value(noise_=noise + h) - value(noise_=noise - h)) / (2 * h)),
             ("nu", g64["nu"].reshape(()), (value(nu_=nu + 1e-5) - value(nu_=nu - 1e-5)) / 2e-5)]
    for r, c in ((ni[0, 0], 0), (ni[1, k - 1], 3), (ni[3, 2], 1)):
        pairs.append((f"Xn[{r},{c}]", g64["Xn"][r, c], (value(Xn_=shifted(Xn, r, c, h)) - value(Xn_=shifted(Xn, r, c, -h))) / (2 * h)))
        pairs.append((f"Y[{r},{c % 2}]", g64["Y"][r, c % 2],
                      (value(Y_=shifted(Y, r, c % 2, h)) - value(Y_=shifted(Y, r, c % 2, -h))) / (2 * h)))
    if not shared:
        for i in (0, 4):
            r = bi[i]
            pairs.append((f"Xq[{r},2]", g64["Xq"][r, 2], (value(Xq_=shifted(Xq, r, 2, h)) - value(Xq_=shifted(Xq, r, 2, -h))) / (2 * h)))
    else:
        r = bi[2]  # (one table: the row's gradient carries both roles)
        pairs.append((f"X[{r},2]", g64["Xn"][r, 2], (value(Xn_=shifted(Xn, r, 2, h)) - value(Xn_=shifted(Xn, r, 2, -h))) / (2 * h)))
    scale = max(abs(fd) for _, _, fd in pairs)
    for name, got, fd in pairs:
        print(f"k = {k}: {name} analytic {float(got)!r} against central difference {fd!r}")
        np.testing.assert_allclose(got, fd, rtol=2e-6, atol=2e-7 * scale, err_msg=name)
    _, _, g32 = _autograd_run("float32", Xq, Xn, Y, bi, ni, gm, gv, ls, noise, nu, shared)
    for name, g in g32.items():
        if g is None or (shared and name == "Xq"):
            continue
        assert np.isfinite(g).all(), name
        assert_close(g, g64[name], GRAD_RTOL["float32"], f"fp32 against fp64: {name}")


def test_autograd_posterior_with_a_float_smoothness_runs_without_the_nu_derivative():
    Xq, Xn, Y, bi, ni, gm, gv = _autograd_problem(12, False)
    _, _, with_nu = _autograd_run("float64", Xq, Xn, Y, bi, ni, gm, gv, 0.6, NUGGET, 1.3, False)
    _, _, grads = _autograd_run("float64", Xq, Xn, Y, bi, ni, gm, gv, 0.6, NUGGET, 1.3, False, nu_tensor=False)
    assert grads["nu"] is None  # (... and _autograd_run has seen the instantiation without dk/dnu serve it)
    for name in ("Xq", "Xn", "Y", "ls", "noise"):
        np.testing.assert_allclose(grads[name], with_nu[name], rtol=1e-9, atol=1e-12)


def test_autograd_posterior_refusals_name_the_limit():
    from muygpys_amd import autograd, fused

    t = torch.float64
    k = limit("float64") + 1
    Xq, Xn, Y, bi, ni, _, _ = _autograd_problem(k, False)
    args = (to_dev(Xq, t), to_dev(Xn, t), to_dev(bi), to_dev(ni), to_dev(Y, t))
    for beyond in (None, True):
        with pytest.raises(ValueError, match=f"limit {limit('float64')}"):
            autograd.posterior(fused.KernelSpec("matern_gen", "l2", 0.6, NUGGET, smoothness=1.3), *args, beyond_lds=beyond)
    small = (args[0], args[1], args[2], args[3][:, :10].contiguous(), args[4])
    with pytest.raises(ValueError, match="nu <= 30"):
        autograd.posterior(fused.KernelSpec("matern_gen", "l2", 0.6, NUGGET, smoothness=30.5), *small)
    for nu in (0.0, -1.0):
        with pytest.raises(ValueError, match="nu > 0"):
            autograd.posterior(fused.KernelSpec("matern_gen", "l2", 0.6, NUGGET, smoothness=nu), *small)
