"""The general-smoothness Matern beyond 64 slots: the general-nu instantiations of the two workgroup kernel families
(csrc/mgp_generic.hip: the system in LDS; csrc/mgp_large.hip: the system in a slab of global memory) against a numpy
fp64 oracle -- oracle.muygps_oracle with ``matern_gen_fn`` (scipy ``kv``) and ``np.linalg.solve`` -- at the project's
tolerances (tests/util.py: fp64 1e-5, fp32 1e-3).

Inputs: the recipe of tests/test_gpu_large.py -- uniform [0, 1]^d points, length scale 0.5, nugget 1e-2, responses
sin(3 sum x) + 0.1 noise -- and nu in {0.42, 1.0, 2.2, 3.7, 8.0}.  Two pairings are excluded, for reasons of the model and
of the fp32 arithmetic, not of the kernels:
  * the F2 metric goes with nu <= 0.5 only (a Matern of higher smoothness on SQUARED distances is not positive
    definite: the comment in tests/test_gpu_large.py); the smallest eigenvalue of the oracle's matrices is checked below;
  * nu = 8 stays out of the d <= 3 cases in either width (one rule for the case lists): there the fp32 evaluator's own
    error (<= 3e-5 absolute up to nu = 25, csrc/mgp_wave_common.h) moves the fp64 solution by up to three quarters of
    the fp32 tolerance, which leaves the fp32 factorisation no room;
  * for the same reason d = 1 with nn_count >= 31 (a tenth and more of the 300 table rows, all on one line) runs in
    fp64 only: the evaluator's error alone moves those fp32 solutions by up to half the tolerance (5e-4 measured by the
    check below at nn_count 32 and 99); nn_count 1 and 2 cover d = 1 in fp32;
  * F2 is not paired with d = 70: at length scale 0.5 the squared distances are ~47 length scales, every covariance is
    below 1e-18 and the posterior mean is of the order 1e-13 -- nothing a relative tolerance can be asked of.
``test_fp32_cases_are_well_conditioned`` (no GPU) keeps the case lists honest: with the oracle's kernel replaced by the
numpy-float32 restatement of the kernel's arithmetic (tests/test_matern_gen_cpu.py::_matern_gen_trapezoid_fp32) and the
solve still in fp64, mean, variance and y^T K^-1 y of every fp32 case move by at most a quarter of the tolerance."""

import numpy as np
import pytest
import torch

from oracle import muygps_oracle as orc
from tests.util import RTOL, assert_close, assert_rel_close, to_dev

gpu = pytest.mark.gpu

TORCH = {"float32": torch.float32, "float64": torch.float64}
CTYPE = {"float32": "float", "float64": "double"}
NUS = (0.42, 1.0, 2.2, 3.7, 8.0)
LS, NUGGET = 0.5, 1e-2
N_ROWS, BATCH = 300, 37
LDS_KERNEL, SLAB_KERNEL = "mgp::fused_generic_gen_kernel<{}>", "mgp::fused_large_gen_kernel<{}>"

# Covariance strip = workgroup size x pairs per evaluator call (gen_pairs_per_call, csrc/mgp_gen_launch.h: 4 in fp32, 2
# in fp64).  Workgroup sizes: 64 (k + 1 + R <= 64) / 256 in the LDS family (lds_factor_threads), 256 (k + 1 + R <= 128) /
# 512 in the slab family (slab_block_threads) -- strips of 256 / 1024 / 2048 pairs in fp32 and 128 / 512 / 1024 in fp64.
# Every strip is a power of two, 2^s, and grows with k, so the pair count k (k + 1) / 2 can land
#   * ON a multiple only where 2^(s+1) divides k or k + 1, i.e. k + 1 >= twice the strip: never (the strip is at least
#     (k + 1 + R) / 2 in both families);
#   * ONE ABOVE a multiple only where 2^(s+1) divides (k - 1)(k + 2): k = 1 (one pair: one above zero), else never;
#   * ONE BELOW a multiple where k^2 + k + 2 = 0 mod 2^(s+1): k = 90 (4095 pairs = 4 x 1024 - 1 = 8 x 512 - 1) in both
#     families and both widths, and no other k <= 1022.
# The nearest the other k come to an edge: k = 55 (1540 pairs: 4 above 6 x 256 and 12 x 128, the 64-thread strips, and
# above 3 x 512), k = 78 (3081: 9 above 3 x 1024 and 6 x 512), and in the 512-thread strips of the slab family k = 239
# (28680: 8 above 14 x 2048 and 28 x 1024) and k = 271 (36856: 8 below 18 x 2048 and 36 x 1024).
STRIP_EDGE_K = {"both": (55, 78, 90), "large": (239, 271)}


def make_table(rng, n, d, R=1):
    X = rng.uniform(size=(n, d))
    Y = np.stack([np.sin(3.0 * X.sum(1) + r) + 0.1 * rng.normal(size=n) for r in range(R)], axis=1)
    return X, Y


def neighbourhoods(rng, n, b, k):
    return np.stack([rng.choice(n, size=k, replace=False) for _ in range(b)])


def gen_spec(nu, metric, ls, noise, fn=None):
    """The oracle's model: scipy's kv through matern_gen_fn, or ``fn(scaled distances, nu)`` in its place."""
    fn = fn or orc.matern_gen_fn
    return orc.Spec(lambda r: fn(r, nu), metric, ls, noise)


def oracle_outputs(ospec, Xq, Xn, bi, ni, Y, noise_rows=None, want_kin=False):
    """mean (b, R), var (b,), ykinvy (b, R) in fp64, as tests/test_gpu_large.py::oracle_outputs computes them."""
    cd = orc.crosswise_tensor(Xq, Xn, bi, ni)
    pd = orc.pairwise_tensor(Xn, ni)
    Kc, Kin = orc.kernel_tensors(ospec, cd, pd)
    if noise_rows is not None:
        Kin = Kin + np.stack([np.diag(r) for r in noise_rows])
    else:
        Kin = orc.perturb(ospec, Kin, ni)
    Yn = Y[ni]
    A = np.linalg.solve(Kin, np.concatenate([Kc[:, :, None], Yn], axis=2))
    mean = np.einsum("bk,bkr->br", Kc, A[:, :, 1:])
    var = 1.0 - np.einsum("bk,bk->b", Kc, A[:, :, 0])
    yk = np.einsum("bkr,bkr->br", Yn, A[:, :, 1:])
    return (mean, var, yk, Kin) if want_kin else (mean, var, yk)


def check(got, ref, dtype, what):
    (mean, var, yk), (m_ref, v_ref, y_ref) = got, ref
    torch.cuda.synchronize()
    rtol = RTOL[dtype]
    mean, var, yk = (x.double().cpu().numpy() for x in (mean, var, yk))
    print(f"{what}: max |mean - ref| {np.abs(mean.reshape(m_ref.shape) - m_ref).max():.3e}, "
          f"max rel var {np.abs(var / v_ref - 1).max():.3e}, max rel ykinvy {np.abs(yk.reshape(y_ref.shape) / y_ref - 1).max():.3e}")
    assert_close(mean.reshape(m_ref.shape), m_ref, rtol, f"{what}: mean")
    assert_rel_close(var, v_ref, rtol, f"{what}: var")
    assert_rel_close(yk.reshape(y_ref.shape), y_ref, rtol, f"{what}: ykinvy")


def max_gen(dtype, R=1):
    from muygpys_amd import _lib

    return _lib.load().mgp_max_nn_count_gen(4 if dtype == "float32" else 8, R)


# ---- the case lists ------------------------------------------------------------------------------------------------
EDGE_K = (1, 2, 31, 32, 33, 67, 99)
EDGE_R = (1, 3, 16)
EDGE_D = (1, 3, 8, 40, 70)


def _edge_cases():
    """A seeded sample in which every value of every factor appears (as tests/test_gpu_large.py::_edge_cases), each case
    run through both families by name; plus the nn_counts at the strip edges above."""
    rng = np.random.default_rng(20261020)
    n_cases = 30

    def spread(values):
        reps = -(-n_cases // len(values))
        return [values[i] for i in rng.permutation(np.tile(np.arange(len(values)), reps))[:n_cases]]

    cols = dict(k=spread(EDGE_K), R=spread(EDGE_R), d=spread(EDGE_D), nu=spread(NUS), metric=spread(["l2", "F2"]),
                aniso=spread([False, True]), noise=spread(["scalar", "table", "batch"]), gathered=spread([False, True]),
                bi=spread([True, False]), own_query=spread([False, True]), dtype=spread(["float32", "float64"]))
    cases = [{name: vals[i] for name, vals in cols.items()} for i in range(n_cases)]
    for i, c in enumerate(cases):
        c["families"] = ("generic", "large")
        if c["d"] <= 3 and c["nu"] == 8.0:
            c["nu"] = NUS[i % 4]
        if c["d"] == 70:
            c["metric"] = "l2"  # (F2 there: squared distances of ~47 length scales, covariances below 1e-18, means of 1e-13)
        if c["metric"] == "F2":  # (squared distances: the roughest smoothness only)
            c["nu"] = 0.42
        if c["d"] == 1 and c["k"] > 2:
            c["dtype"] = "float64"  # (30 and more of 300 points on a line: see test_fp32_cases_are_well_conditioned)
    j = 0
    for families, ks in (("generic", "large"), STRIP_EDGE_K["both"]), (("large",), STRIP_EDGE_K["large"]):
        for k in ks:
            for dtype in ("float32", "float64"):
                cases.append(dict(k=k, R=1, d=8, nu=NUS[j % 5], metric="l2", aniso=bool(j % 2), noise="scalar", gathered=False,
                                  bi=True, own_query=False, dtype=dtype, families=families))
                j += 1
    return cases


EDGE_CASES = _edge_cases()

# (dtype, k, R, d, b, nu, kernel the dispatcher must choose); k: a number, or relative to mgp_max_nn_count_gen(es, 1)
ROUTING_CASES = [(dtype, k, 1, 8, b, nu, kernel) for dtype in ("float32", "float64") for k, b, nu, kernel in (
    (63, 37, 2.2, LDS_KERNEL), ("max_gen", 8, 0.42, LDS_KERNEL), ("max_gen+1", 8, 3.7, SLAB_KERNEL))]
ROUTING_CASES.append(("float32", 1022, 1, 8, 4, 1.0, SLAB_KERNEL))


def _edge_id(c):
    return (f"k{c['k']}-R{c['R']}-d{c['d']}-nu{c['nu']}-{c['metric']}-{'aniso' if c['aniso'] else 'iso'}-{c['noise']}"
            f"-{'gathered' if c['gathered'] else 'table'}-{'bi' if c['bi'] else 'nobi'}-{'q' if c['own_query'] else 'same'}-{c['dtype']}")


def edge_inputs(c):
    """Everything of an edge case in numpy, from a seed of its own."""
    rng = np.random.default_rng(sum(map(ord, _edge_id(c))))
    k, R, d, b = c["k"], c["R"], c["d"], BATCH
    n, nq = max(N_ROWS, k + 30), 53
    Xn, Y = make_table(rng, n, d, R)
    Xq = make_table(rng, nq, d)[0] if c["own_query"] else Xn
    ni = neighbourhoods(rng, n, b, k)
    bi = rng.choice(Xq.shape[0], size=b, replace=False) if c["bi"] else np.arange(b)
    ls = LS * (1.0 + 0.3 * rng.uniform(size=d)) if c["aniso"] else LS
    table = NUGGET * (1.0 + rng.uniform(size=n))
    return dict(Xn=Xn, Y=Y, Xq=Xq, ni=ni, bi=bi, ls=ls, table=table, noise=NUGGET if c["noise"] == "scalar" else table)


def routing_inputs(dtype, k, R, d, b, nu):
    k = {"max_gen": max_gen(dtype), "max_gen+1": max_gen(dtype) + 1}.get(k, k)
    rng = np.random.default_rng(k * 7 + R)
    n = 1500
    X, Y = make_table(rng, n, d, R)
    return k, X, Y, neighbourhoods(rng, n, b, k), rng.choice(n, size=b, replace=False)


# ---- no GPU: the lists themselves ----------------------------------------------------------------------------------
def test_edge_sample_covers_every_factor():
    seen = {name: {c[name] for c in EDGE_CASES} for name in EDGE_CASES[0]}
    assert set(EDGE_K) | set(STRIP_EDGE_K["both"]) | set(STRIP_EDGE_K["large"]) <= seen["k"]
    assert seen["R"] == set(EDGE_R) and seen["d"] == set(EDGE_D) and seen["nu"] == set(NUS)
    assert seen["metric"] == {"l2", "F2"} and seen["noise"] == {"scalar", "table", "batch"}
    for name in ("aniso", "gathered", "bi", "own_query"):
        assert seen[name] == {False, True}, name
    assert seen["dtype"] == {"float32", "float64"}
    assert all(c["nu"] <= 0.5 for c in EDGE_CASES if c["metric"] == "F2")
    assert not any(c["nu"] == 8.0 and c["d"] <= 3 for c in EDGE_CASES)
    # the strip arithmetic of the comment above
    for k, strips, off in ((90, (1024, 512), -1), (55, (256, 128, 512), 4), (78, (1024, 512), 9), (239, (2048, 1024), 8), (271, (2048, 1024), -8)):
        assert all((k * (k + 1) // 2 - off) % s == 0 for s in strips), k


def test_strip_edge_counts_against_the_launch_rules():
    """k = 90 is the one nn_count whose pair count sits next to a strip edge: searched, not assumed."""
    def threads(family, rows):
        return (64 if rows <= 64 else 256) if family == "generic" else (256 if rows <= 128 else 512)

    hits = set()
    for family, kmax in (("generic", 192), ("large", 1022)):
        for per_call in (4, 2):
            for k in range(2, kmax + 1):
                strip, pairs = threads(family, k + 2) * per_call, k * (k + 1) // 2
                if pairs >= strip - 1 and (pairs + 1) % strip <= 2:  # one below, on, one above
                    hits.add((k, (pairs + 1) % strip - 1))
    assert hits == {(90, -1)}, hits


def _shift(ref, alt):
    """The largest move of (mean, var, ykinvy) in units of the tolerance's own measure: the rms-augmented bound of
    assert_close for the mean, the relative bound of assert_rel_close for the other two (rtol = 1)."""
    (m, v, y), (m2, v2, y2) = ref, alt
    rms = float(np.sqrt(np.mean(m**2)))
    return max(float((np.abs(m2 - m) / (np.abs(m) + rms)).max()), float(np.abs(v2 / v - 1).max()), float(np.abs(y2 / y - 1).max()))


def _fp32_kernel(r, nu):
    """The fp32 evaluator's arithmetic on the off-diagonal distances (the kernels never evaluate the diagonal, and a zero
    distance is 1 by rule: neither drives the node count)."""
    from tests.test_matern_gen_cpu import _matern_gen_trapezoid_fp32

    r = np.asarray(r, dtype=np.float64)
    out = np.ones_like(r)
    if (r > 0).any():
        out[r > 0] = _matern_gen_trapezoid_fp32(r[r > 0], nu)[0]
    return out


def test_fp32_cases_are_well_conditioned():
    """Every fp32 case of the lists: the evaluator's own error moves the fp64 solution by at most a quarter of the fp32
    tolerance; every F2 case: the oracle's matrices are positive definite."""
    worst = {}
    for c in EDGE_CASES:
        if c["dtype"] != "float32" and c["metric"] != "F2":
            continue
        x = edge_inputs(c)
        ref = oracle_outputs(gen_spec(c["nu"], c["metric"], x["ls"], x["noise"]), x["Xq"], x["Xn"], x["bi"], x["ni"], x["Y"], want_kin=True)
        if c["metric"] == "F2":
            lam = float(np.linalg.eigvalsh(ref[3]).min())
            assert lam > 0.5 * NUGGET, (_edge_id(c), lam)
        if c["dtype"] == "float32":
            alt = oracle_outputs(gen_spec(c["nu"], c["metric"], x["ls"], x["noise"], _fp32_kernel), x["Xq"], x["Xn"], x["bi"], x["ni"], x["Y"])
            worst[_edge_id(c)] = _shift(ref[:3], alt)
    for dtype, k, R, d, b, nu, _ in ROUTING_CASES:
        if dtype == "float32":
            k, X, Y, ni, bi = routing_inputs(dtype, k, R, d, b, nu)
            ref = oracle_outputs(gen_spec(nu, "l2", LS, NUGGET), X, X, bi, ni, Y)
            worst[f"routing k{k} nu{nu}"] = _shift(ref, oracle_outputs(gen_spec(nu, "l2", LS, NUGGET, _fp32_kernel), X, X, bi, ni, Y))
    top = sorted(worst.items(), key=lambda kv: -kv[1])[:3]
    print("largest shifts:", top)
    assert top[0][1] <= 0.25 * RTOL["float32"], top


# ---- 1. edges through both families by name ------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("c", EDGE_CASES, ids=[_edge_id(c) for c in EDGE_CASES])
def test_edges_through_both_families(c):
    from muygpys_amd import _lib
    from muygpys_amd.fused import KernelSpec, posterior_mean_var

    x = edge_inputs(c)
    dtype, t = c["dtype"], TORCH[c["dtype"]]
    ref = oracle_outputs(gen_spec(c["nu"], c["metric"], x["ls"], x["noise"]), x["Xq"], x["Xn"], x["bi"], x["ni"], x["Y"])
    d_noise = NUGGET if c["noise"] == "scalar" else to_dev(x["table"] if c["noise"] == "table" else x["table"][x["ni"]], t)
    Xn_d, Y_d = to_dev(x["Xn"], t), to_dev(x["Y"], t)
    Xq_d = to_dev(x["Xq"], t) if c["own_query"] else Xn_d
    tg = Y_d[to_dev(x["ni"])] if c["gathered"] else Y_d
    spec = KernelSpec("matern_gen", c["metric"], list(x["ls"]) if c["aniso"] else x["ls"], d_noise, smoothness=c["nu"])
    for family, name in (("generic", LDS_KERNEL), ("large", SLAB_KERNEL)):
        if family not in c["families"]:
            continue
        info = torch.zeros(1, dtype=torch.int32, device="cuda")
        got = posterior_mean_var(spec, Xq_d, Xn_d, to_dev(x["bi"]) if c["bi"] else None, to_dev(x["ni"]), tg, want_ykinvy=True,
                                 info=info, path=family, gathered=c["gathered"])
        assert _lib.last_kernel() == name.format(CTYPE[dtype])
        check(got, ref, dtype, f"{family}: {_edge_id(c)}")
        assert int(info.item()) == 0


# ---- 2. routing on path="auto" -------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("dtype, k, R, d, b, nu, kernel", ROUTING_CASES, ids=[f"{c[0]}-k{c[1]}-nu{c[5]}" for c in ROUTING_CASES])
def test_routing_on_auto(dtype, k, R, d, b, nu, kernel):
    from muygpys_amd import _lib
    from muygpys_amd.fused import KernelSpec, posterior_mean_var

    k, X, Y, ni, bi = routing_inputs(dtype, k, R, d, b, nu)
    ref = oracle_outputs(gen_spec(nu, "l2", LS, NUGGET), X, X, bi, ni, Y)
    t = TORCH[dtype]
    Xd = to_dev(X, t)
    info = torch.zeros(1, dtype=torch.int32, device="cuda")
    got = posterior_mean_var(KernelSpec("matern_gen", "l2", LS, NUGGET, smoothness=nu), Xd, Xd, to_dev(bi), to_dev(ni), to_dev(Y, t),
                             want_ykinvy=True, info=info)
    assert _lib.last_kernel() == kernel.format(CTYPE[dtype])
    check(got, ref, dtype, f"auto, k = {k}")
    assert int(info.item()) == 0


@gpu
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_more_than_1024_rows_is_fused_unsupported(dtype):
    from muygpys_amd.fused import FusedUnsupported, KernelSpec, posterior_mean_var

    rng = np.random.default_rng(1023)
    n, d, k = 1100, 4, 1023
    t = TORCH[dtype]
    X, y = to_dev(rng.uniform(size=(n, d)), t), to_dev(rng.normal(size=n), t)
    with pytest.raises(FusedUnsupported):
        posterior_mean_var(KernelSpec("matern_gen", "l2", LS, NUGGET, smoothness=1.0), X, X, to_dev(np.arange(2)),
                           to_dev(neighbourhoods(rng, n, 2, k)), y)


# ---- 3. the general form at nu = 1/2, 3/2, 5/2 against the closed form of the same family ----------------------------------
@gpu
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("k", [80, "max_gen+1"])
@pytest.mark.parametrize("nu, closed", [(0.5, "matern05"), (1.5, "matern15"), (2.5, "matern25")])
def test_general_form_agrees_with_the_closed_form(nu, closed, k, dtype):
    from muygpys_amd import _lib
    from muygpys_amd.fused import KernelSpec, posterior_mean_var

    family = "generic" if k == 80 else "large"
    k = max_gen(dtype) + 1 if k == "max_gen+1" else k
    rng = np.random.default_rng(k)
    n, d, b = 1500, 8, 8
    X, Y = make_table(rng, n, d)
    t = TORCH[dtype]
    args = (to_dev(X, t), to_dev(X, t), to_dev(rng.choice(n, size=b, replace=False)), to_dev(neighbourhoods(rng, n, b, k)), to_dev(Y, t))
    general = posterior_mean_var(KernelSpec("matern_gen", "l2", LS, NUGGET, smoothness=nu), *args, want_ykinvy=True, path=family)
    assert _lib.last_kernel() == (LDS_KERNEL if family == "generic" else SLAB_KERNEL).format(CTYPE[dtype])
    closed_form = posterior_mean_var(KernelSpec(closed, "l2", LS, NUGGET), *args, want_ykinvy=True, path=family)
    assert _lib.last_kernel() == f"mgp::fused_{family}_kernel<{CTYPE[dtype]}>"
    torch.cuda.synchronize()
    check(general, tuple(x.double().cpu().numpy() for x in closed_form), dtype, f"nu = {nu} against {closed}, k = {k}")


# ---- 4. placement ----------------------------------------------------------------------------------------------------
def _direct_large(Xd, Yd, d, bi, ni, k, nu, slabs):
    """mgp_posterior_gen_large_* itself on a workspace of `slabs` slabs (None: the recommended size)."""
    from muygpys_amd import _lib

    lib, es, t, m = _lib.load(), Xd.element_size(), Xd.dtype, len(bi)
    size = lib.mgp_large_workspace_bytes(es, k, 1, m) if slabs is None else slabs * lib.mgp_large_workspace_bytes(es, k, 1, 1)
    ws = torch.empty(size, dtype=torch.uint8, device="cuda")
    ws.fill_(0xFF)  # (what the slab held before must not matter: NaN in every element, either width)
    bi_d, ni_d, ls = to_dev(bi), to_dev(ni), torch.tensor([LS], device="cuda", dtype=t)
    outs = [torch.empty(m, device="cuda", dtype=t) for _ in range(3)]
    P = _lib.ptr
    rc = _lib.fn("posterior_gen_large", t)(P(Xd), P(Xd), d, P(bi_d), P(ni_d), m, k, P(Yd), 1, 0, 0, NUGGET, None, float(nu), 0, P(ls), 1,
                                           P(outs[0]), P(outs[1]), P(outs[2]), None, P(ws), size, _lib.stream_ptr())
    assert rc == 0
    torch.cuda.synchronize()
    return [x.cpu().numpy() for x in outs]


@gpu
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("family, k", [("generic", 90), ("large", 140)])
def test_placement_invariance_bitwise(family, k, dtype):
    """A neighbourhood's bits do not depend on its place in the batch, the batch size, the grid or the workspace: the
    pair-to-thread map of the covariance phase -- and with it the node count of every pair's wave -- is a function of
    nn_count and the workgroup size alone."""
    from muygpys_amd.fused import KernelSpec, posterior_mean_var

    rng = np.random.default_rng(k)
    n, d, nu = 1200, 8, 2.2
    X, Y = make_table(rng, n, d)
    ni = neighbourhoods(rng, n, 205, k)  # 200 unrelated neighbourhoods, then the 5 under test
    bi = rng.choice(n, size=205, replace=False)
    t = TORCH[dtype]
    Xd, Yd, spec = to_dev(X, t), to_dev(Y[:, 0], t), KernelSpec("matern_gen", "l2", LS, NUGGET, smoothness=nu)

    def fused(rows):
        out = posterior_mean_var(spec, Xd, Xd, to_dev(bi[rows]), to_dev(ni[rows]), Yd, want_ykinvy=True, path=family)
        torch.cuda.synchronize()
        return [x.cpu().numpy() for x in out]

    whole = fused(np.arange(205))
    for j in range(200, 205):
        alone = fused(np.array([j]))
        for a, w, what in zip(alone, whole, ("mean", "var", "ykinvy")):
            assert np.isfinite(a[0]) and a[0].tobytes() == w[j].tobytes(), (j, what, a[0], w[j])
    if family == "large":
        rows = np.arange(198, 205)
        one_slab = _direct_large(Xd, Yd, d, bi[rows], ni[rows], k, nu, 1)
        recommended = _direct_large(Xd, Yd, d, bi[rows], ni[rows], k, nu, None)
        for o, r, w in zip(one_slab, recommended, whole):
            assert o.tobytes() == r.tobytes() == w[rows].tobytes()


# ---- 5. degenerate inputs --------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("family, k", [("generic", 70), ("large", 140)])
def test_degenerate_inputs(family, k, dtype):
    """A duplicated neighbour row: k(0) follows the evaluators' own rules -- fp32: exactly 1; fp64: the reference's eps
    nudge, evaluated like any other distance.  With the nugget the system is well posed and must match the oracle.
    Without it the duplicate in columns 0 and 1 gives the second pivot 1 - K_10^2: exactly zero in fp32, so the
    neighbourhood is counted and NaN; in fp64 K_10 = k(eps) is 1 up to the evaluator's 6e-13, the sign of the pivot is
    decided by rounding, and either outcome -- counted and NaN, or neither -- is consistent (measured on gfx950 at
    nu = 2.2: info = 0 and finite outputs in both families); the batch-mates are untouched in both.  A NaN feature: NaN
    for that neighbourhood only, and the launch returns."""
    from muygpys_amd.fused import KernelSpec, posterior_mean_var

    rng = np.random.default_rng(k + 5)
    n, d, b, nu = 1000, 8, 8, 2.2
    X, Y = make_table(rng, n, d)
    ni = neighbourhoods(rng, n - 1, b, k)  # (row n - 1 belongs to the NaN experiment alone)
    bi = rng.choice(n - 1, size=b, replace=False)
    dup = 2
    ni[dup, 1] = ni[dup, 0]
    t = TORCH[dtype]
    Xd, yd = to_dev(X, t), to_dev(Y[:, 0], t)

    def run(noise, X_dev=Xd, nn=ni):
        info = torch.zeros(1, dtype=torch.int32, device="cuda")
        out = posterior_mean_var(KernelSpec("matern_gen", "l2", LS, noise, smoothness=nu), X_dev, X_dev, to_dev(bi), to_dev(nn), yd,
                                 want_ykinvy=True, info=info, path=family)
        torch.cuda.synchronize()
        return out, int(info.item())

    # with the nugget: finite, and the oracle's
    got, bad = run(NUGGET)
    assert bad == 0 and all(torch.isfinite(x).all() for x in got)
    check(got, oracle_outputs(gen_spec(nu, "l2", LS, NUGGET), X, X, bi, ni, Y), dtype, "duplicated neighbour, nugget 1e-2")
    # without it, in that one neighbourhood
    noise = np.full((b, k), NUGGET)
    noise[dup] = 0.0
    good = np.setdiff1d(np.arange(b), [dup])
    (mean, var, yk), bad = run(to_dev(noise, t))
    flagged = bool(torch.isnan(mean[dup]).item())
    print(f"{family} {dtype}: duplicated neighbour at nugget 0: info = {bad}, mean = {float(mean[dup])!r}")
    if dtype == "float32":
        assert flagged
    assert bad == int(flagged) and all(bool(torch.isnan(x[dup]).item()) == flagged for x in (mean, var, yk))
    g = to_dev(good)
    ref = oracle_outputs(gen_spec(nu, "l2", LS, 0.0), X, X, bi[good], ni[good], Y, noise_rows=noise[good])
    check((mean[g], var[g], yk[g]), ref, dtype, "the batch-mates of the singular neighbourhood")
    # a NaN feature in a row only neighbourhood 5 holds
    Xn = X.copy()
    Xn[n - 1, 3] = np.nan
    nn = ni.copy()
    nn[5, k // 2] = n - 1
    (mean, var, yk), bad = run(NUGGET, to_dev(Xn, t), nn)
    rest = to_dev(np.setdiff1d(np.arange(b), [5]))
    for x in (mean, var, yk):
        assert torch.isnan(x[5]).all() and torch.isfinite(x[rest]).all()
    assert bad <= 1
    ref = oracle_outputs(gen_spec(nu, "l2", LS, NUGGET), X, X, bi, ni, Y)
    keep = np.setdiff1d(np.arange(b), [5])
    check((mean[rest], var[rest], yk[rest]), tuple(r[keep] for r in ref), dtype, "the batch-mates of the NaN neighbourhood")


# ---- 6. the functor layer --------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_functor_layer_is_one_general_launch(dtype):
    from muygpys_amd import _lib
    from muygpys_amd.gp import MuyGPS
    from muygpys_amd.gp.deformation import Isotropy, l2
    from muygpys_amd.gp.hyperparameter import AnalyticScale, Parameter
    from muygpys_amd.gp.kernels import Matern
    from muygpys_amd.gp.noise import HomoscedasticNoise

    rng = np.random.default_rng(80)
    n, d, k, b, nu = 1200, 8, 80, 37, 0.8
    X, Y = make_table(rng, n, d)
    y = Y[:, 0]
    bi, ni = rng.choice(n, size=b, replace=False), neighbourhoods(rng, n, b, k)
    t = TORCH[dtype]
    rtol = RTOL[dtype]
    Xd, yd, bi_d, ni_d = to_dev(X, t), to_dev(y, t), to_dev(bi), to_dev(ni)
    m = MuyGPS(kernel=Matern(smoothness=Parameter(nu), deformation=Isotropy(l2, Parameter(LS, (0.05, 5.0)))),
               noise=HomoscedasticNoise(NUGGET), scale=AnalyticScale())
    m_ref, v_ref, _ = oracle_outputs(gen_spec(nu, "l2", LS, NUGGET), X, X, bi, ni, y[:, None])
    cross, pair, y_nn = m.make_predict_tensors(bi_d, ni_d, Xd, Xd, yd)
    Kin, Kc = m.kernel(pair), m.kernel(cross)
    assert not isinstance(Kin, torch.Tensor)  # lazy handles: nothing materialised
    # (a closed-form launch first, so that the name read below is this evaluation's)
    from muygpys_amd.fused import KernelSpec, posterior_mean_var

    posterior_mean_var(KernelSpec("matern15", "l2", LS, NUGGET), Xd, Xd, bi_d, ni_d[:, :5].contiguous(), yd)
    assert "gen_kernel" not in _lib.last_kernel()
    mean = m.posterior_mean(Kin, Kc, y_nn)
    assert _lib.last_kernel() == LDS_KERNEL.format(CTYPE[dtype])
    var = m.posterior_variance(Kin, Kc)
    assert _lib.last_kernel() == LDS_KERNEL.format(CTYPE[dtype])
    torch.cuda.synchronize()
    assert_close(mean.cpu().numpy().reshape(-1), m_ref[:, 0], rtol, "posterior_mean")
    assert_rel_close(var.cpu().numpy().reshape(-1), v_ref * float(m.scale()), rtol, "posterior_variance")
