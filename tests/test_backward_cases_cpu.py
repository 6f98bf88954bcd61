"""What tests/test_gpu_backward_rungs.py relies on, asserted without a GPU: the per-neighbourhood reference of
tests/backward_cases.py is right (its sums over the neighbourhoods are the oracle's posterior_vjp, it reproduces the
reference's own autograd results in tests/golden/grad_*.npz within their pin, and its y^T K^-1 y term is a central
difference of the oracle's), the restated launch rules are the library's, the sample covers what it claims, plain
fp32 arithmetic stays inside half of the fp32 band on every fp32 case, and every wrong reading of an argument moves
the outputs of the case meant to catch it at least ten bands away."""

import glob
import os
from types import SimpleNamespace

import numpy as np
import pytest

from oracle import muygps_oracle as orc
from tests import backward_cases as BC
from tests.conftest import GOLDEN_DIR, grad_spec, load_golden
from tests.util import assert_close

HALF = BC.RTOL["float32"] / 2    # what plain fp32 arithmetic may cost on these inputs
MOVED = 10 * BC.RTOL["float32"]  # what a wrong reading must cost
SHAPE_TAGS = ("shape", "shape-hyper", "shape-feat", "past-limit")
MODE_CASES = [c for c in BC.CASES if c["tag"] not in SHAPE_TAGS and c["b"] != BC.LONG_B]


def _full(c, P):
    """The reference pieces over ALL neighbourhoods (a non-SPD case keeps its good noise here)."""
    return BC.reference(c["id"])[0] if not c["bad"] else BC.vjp_rows(P)


# ---- 1. the reference is right -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", [c["id"] for c in BC.CASES if not c["loocv"]])
def test_sums_over_the_neighbourhoods_are_the_oracle_vjp(cid):
    c, P = BC.BY_ID[cid], BC.problem(cid)
    v = _full(c, P)
    spec = orc.Spec(c["kernel"], c["metric"], P.ls, BC.NOISE if c["noise"] == "scalar" else P.table)
    gm = np.zeros((P.b, c["R"])) if P.gm is None else P.gm
    gv = np.zeros(P.b) if P.gv is None else P.gv
    ref = orc.posterior_vjp(spec, P.Xq, P.Xn, P.bi, P.ni, P.Y, gm, gv)
    gq, gn, gt = np.zeros(P.Xq.shape), np.zeros(P.Xn.shape), np.zeros(P.Y.shape)
    np.add.at(gq, P.bi, v.g_q)
    np.add.at(gn, P.ni, v.g_nn)
    np.add.at(gt, P.ni, v.g_tg)
    assert_close(gq, ref["test_features"], 1e-10, "g_test_features")
    assert_close(gn, ref["train_features"], 1e-10, "g_train_features")
    assert_close(gt, ref["targets"], 1e-10, "g_targets")
    assert_close(v.grad_ls.sum(0), np.atleast_1d(ref["length_scale"]), 1e-10, "g_length_scale")
    if c["noise"] == "scalar":
        assert_close(v.grad_noise.sum().reshape(()), np.asarray(ref["noise"]).reshape(()), 1e-10, "g_noise")
    else:
        g = np.zeros(BC.N)
        np.add.at(g, P.ni, v.grad_noise)
        assert_close(g, ref["noise"], 1e-10, "g_noise table")
        assert np.array_equal(P.noise_rows, P.table[P.ni])


def _rel(a, b):
    scale = np.abs(b).max()
    return np.abs(np.asarray(a) - np.asarray(b)).max() / (scale if scale > 0 else 1.0)


@pytest.mark.parametrize("name", sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN_DIR, "grad_*.npz"))))
def test_reference_reproduces_the_reference_autograd(name):
    """tests/golden/grad_*.npz (the reference's torch backend under autograd) within the pin of
    tests/test_oracle_grad_golden.py."""
    g = load_golden(name)
    meta = g["meta"]
    spec, xq = grad_spec(meta, g)
    Y = g["targets"] if g["targets"].ndim == 2 else g["targets"][:, None]
    gm = g["grad_mean"] if g["grad_mean"].ndim == 2 else g["grad_mean"][:, None]
    ni, bi = g["nn_indices"], g["batch_indices"]
    b, k = ni.shape
    rows = g["noise_table"][ni] if meta["hetero"] else np.full((b, k), float(meta["eps"]))
    P = SimpleNamespace(Xn=g["features"], Xq=xq, Y=Y, ni=ni, bi=bi, ls=spec.length_scale, noise_rows=rows, gm=gm, gv=g["grad_var"], gy=None,
                        b=b, kernel=meta["kernel"], metric=meta["metric"])
    v = BC.vjp_rows(P)
    gq, gn, gt = np.zeros(xq.shape), np.zeros(g["features"].shape), np.zeros(Y.shape)
    np.add.at(gq, bi, v.g_q)
    np.add.at(gn, ni, v.g_nn)
    np.add.at(gt, ni, v.g_tg)
    tol = 1e-6
    if meta["separate_test"]:
        assert _rel(gq, g["g_test_features"]) < tol and _rel(gn, g["g_features"]) < tol
    else:
        assert _rel(gq + gn, g["g_features"]) < tol
    assert _rel(gt.reshape(g["g_targets"].shape), g["g_targets"]) < tol
    assert _rel(v.grad_ls.sum(0), g["g_length_scale"]) < tol
    if meta["hetero"]:
        table = np.zeros(g["noise_table"].shape)
        np.add.at(table, ni, v.grad_noise)
        assert _rel(table, g["g_noise_table"]) < tol
    else:
        assert _rel(v.grad_noise.sum(), g["g_noise"]) < tol


def _oracle_ykinvy(c, P, ls, eps):
    """sum_i gy_i y_i^T K_i^-1 y_i by the fp64 oracle's own pieces."""
    spec = orc.Spec(c["kernel"], c["metric"], ls, eps)
    _, Kin = orc.kernel_tensors(spec, orc.crosswise_tensor(P.Xq, P.Xn, P.bi, P.ni), orc.pairwise_tensor(P.Xn, P.ni))
    Kin = orc.perturb(spec, Kin, P.ni)
    y = P.Y[P.ni][:, :, 0]
    return float(np.sum(P.gy * np.einsum("bk,bk->b", y, np.linalg.solve(Kin, y[:, :, None])[:, :, 0])))


@pytest.mark.parametrize("cid", [c["id"] for c in BC.CASES if c["loocv"] == "yk" and c["rung"] == "L" and c["dtype"] == "float64"])
def test_loocv_term_is_a_central_difference_of_the_oracle(cid):
    c, P = BC.BY_ID[cid], BC.problem(cid)
    v = BC.reference(cid)[0]
    assert P.gy is not None and not P.gm.any() and not P.gv.any()
    h = 1e-6
    eps = BC.NOISE if c["noise"] == "scalar" else P.table
    ls = np.atleast_1d(np.asarray(P.ls, dtype=np.float64))
    for f in range(len(ls))[:: max(1, len(ls) // 3)]:
        lp, lm = ls.copy(), ls.copy()
        lp[f] += h
        lm[f] -= h
        fd = (_oracle_ykinvy(c, P, lp if c["aniso"] else float(lp[0]), eps) - _oracle_ykinvy(c, P, lm if c["aniso"] else float(lm[0]), eps)) / (2 * h)
        assert abs(fd - v.grad_ls.sum(0)[f]) < 1e-6 * max(1.0, abs(fd)), (f, fd, v.grad_ls.sum(0)[f])
    fd = (_oracle_ykinvy(c, P, P.ls, eps + h) - _oracle_ykinvy(c, P, P.ls, eps - h)) / (2 * h)  # (every diagonal entry moves)
    assert abs(fd - v.grad_noise.sum()) < 1e-6 * max(1.0, abs(fd)), (fd, v.grad_noise.sum())


# ---- 2. the restated rules are right -----------------------------------------------------------------------------------
def test_restated_lds_rule_is_the_library_own():
    from muygpys_amd import _lib

    lib = _lib.load()
    assert lib.mgp_max_nn_count_backward(4) == BC.max_nn_count_backward(4) == 137
    assert lib.mgp_max_nn_count_backward(8) == BC.max_nn_count_backward(8) == 96
    assert BC.lds_rule(4, 137, 70) == (256, 8, 9)
    # (fp64, k 90, d 70): 32 features would take 164 880 bytes of the 163 840 a workgroup can have; 24 take 158 928
    assert BC.backward_lds_bytes(8, 90, 32) == 164880 and BC.backward_lds_bytes(8, 90, 24) == 158928
    assert BC.lds_rule(8, 90, 70) == (128, 24, 3)
    assert BC.lds_rule(4, 138, 8) is None and BC.lds_rule(8, 97, 8) is None
    assert [BC.lds_rule(4, k, 4)[0] for k in (62, 63, 126, 127)] == [64, 128, 128, 256]


def test_restated_prepared_shapes_are_the_build_own():
    from muygpys_amd import build

    assert tuple(build.PREWARM_BWD) == BC.PREWARM_BWD and len(BC.PREWARM_BWD) == 12
    assert len(BC.ON_DEMAND_BWD) <= 6 and not set(BC.ON_DEMAND_BWD) & set(BC.PREWARM_BWD + BC.BUILTIN_BWD)


# ---- 3. the sample covers what it claims -------------------------------------------------------------------------------
def _expects(rung, dtype=None):
    return [c["expect"] for c in BC.rung_cases(rung) if dtype in (None, c["dtype"]) and c["expect"]]


def test_every_wave_instantiation_appears():
    names = {n for n in _expects("W") if n.startswith("mgp::backward_wave_kernel<")}
    want = set()
    for hyper in ("false", "true"):
        for np_, dgs in ((32, ("4,0", "8,0", "10,0", "10,30", "12,0", "16,0")), (64, ("4,0", "8,0", "10,0", "12,0", "16,0"))):
            want |= {f"mgp::backward_wave_kernel<float,{np_},{dg},{hyper}>" for dg in dgs}
        want |= {f"mgp::backward_wave_kernel<double,{np_},{dg},0,{hyper}>" for np_, dg in ((32, 4), (32, 8), (64, 4))}
    assert len(want) == 28 and names == want, sorted(want ^ names)
    # the shapes of the issue, and the two that must name L
    shapes = {(c["dtype"], c["k"], c["d"]) for c in BC.rung_cases("W") if c["tag"] == "shape"}
    assert {("float32", 1, 1), ("float32", 2, 3), ("float32", 30, 37), ("float32", 62, 64), ("float64", 62, 1), ("float64", 3, 15)} <= shapes
    for k, d in ((31, 9), (40, 16)):
        assert all(c["expect"].startswith("mgp::backward_kernel<double>") for c in BC.rung_cases("W")
                   if (c["dtype"], c["k"], c["d"]) == ("float64", k, d))
    # every instantiation with all outputs and, anisotropic, with grad_ls and grad_noise alone; vectorised or not
    assert any(c["d"] % 4 for c in BC.rung_cases("W") if c["dtype"] == "float32") and any(c["d"] % 2 for c in BC.rung_cases("W") if c["dtype"] == "float64")


def test_forward_kernel_rung_appears_built_in_and_in_both_forms():
    names = _expects("F")
    bwd = "false,backward>"
    assert names.count(f"mgp::fused_wave_kernel<float,32,30,1,40,true,false,false,true,{bwd}") >= 2
    assert names.count(f"mgp::fused_wave_kernel<double,64,50,1,8,true,false,false,false,{bwd}") >= 2
    jit = [n for n in names if n.endswith("[run-time compiled]")]
    for prefix in ("float,32,", "float,64,", "double,32,", "double,64,"):  # row per lane in 32 and 64 slots, the dealt triangle (double, 64)
        assert any(n.startswith("mgp::fused_wave_kernel<" + prefix) for n in jit), prefix
    kinds = {}
    for c in BC.rung_cases("F"):
        kind = BC.prepared_shape(c)
        if kind:
            kinds.setdefault(kind, set()).add((BC.ES[c["dtype"]], c["k"], c["d"]))
    assert kinds["builtin"] == set(BC.BUILTIN_BWD) and kinds["prewarm"] == set(BC.PREWARM_BWD) and kinds["demand"] == set(BC.ON_DEMAND_BWD)
    # the dealt-triangle shapes ask for hyper-parameter outputs only; a request for feature cotangents there names W or L
    for c in BC.rung_cases("F"):
        f = BC.fwd_rule(BC.ES[c["dtype"]], c["k"], c["d"], False, c["kernel"], True)
        if f and f[3] and c["want"] in ("all", "nn"):
            assert "fused_wave_kernel" not in c["expect"], c["id"]
        if c["off"]:
            assert "fused_wave_kernel" not in c["expect"], c["id"]
    assert sum(1 for c in BC.rung_cases("F") if c["tag"] == "shape-feat") >= 5


def test_lds_rung_appears_at_every_thread_count_and_chunking():
    seen = set()
    for c in BC.rung_cases("L"):
        if c["expect"] is None:
            assert (c["dtype"], c["k"]) in (("float32", 138), ("float64", 97))
            continue
        es = BC.ES[c["dtype"]]
        threads, dc, chunks = BC.lds_rule(es, c["k"], c["d"])
        assert c["expect"] == f"mgp::backward_kernel<{BC.CNAME[c['dtype']]}> [threads={threads},dc={dc}]"
        last = c["d"] - (chunks - 1) * dc
        seen.add((c["dtype"], threads, min(chunks, 3), bool(last % (16 // es))))
    for dtype, counts in (("float32", (64, 128, 256)), ("float64", (64, 128))):
        assert {t for dt, t, _, _ in seen if dt == dtype} == set(counts)  # (64 threads: the single-wave solve)
        assert {n for dt, _, n, _ in seen if dt == dtype} == {1, 2, 3}
        for chunks in (1, 2, 3):
            assert any(odd for dt, _, n, odd in seen if dt == dtype and n == chunks), (dtype, chunks)
    shapes = {(c["dtype"], c["k"], c["d"]) for c in BC.rung_cases("L")}
    assert {("float32", 137, 70), ("float64", 90, 70), ("float32", 126, 4), ("float32", 127, 4), ("float64", 96, 6), ("float32", 1, 3)} <= shapes
    assert {d for dt, k, d in shapes if k == 20} == {1, 7, 8, 9, 64, 65, 70}
    assert len(_expects("L")) + 2 == len(BC.rung_cases("L"))


@pytest.mark.parametrize("rung", BC.RUNGS)
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_every_rung_sees_every_mode(rung, dtype):
    cases = [c for c in BC.rung_cases(rung) if c["dtype"] == dtype]
    assert {c["noise"] for c in cases} == {"scalar", "table", "batch"}
    assert {c["bi"] for c in cases} == {True, False} and {c["aniso"] for c in cases} == {True, False}
    assert any(c["own_query"] and c["want"] == "all" for c in cases) and any(not c["own_query"] and c["want"] == "all" for c in cases)
    assert {c["R"] for c in cases} >= {1, 2, 5}
    assert any(not c["gm"] for c in cases) and any(not c["gv"] for c in cases)
    assert {c["want"] for c in cases} >= {"all", "hyper", "nn"} and {c["loocv"] for c in cases} == {None, "all", "yk"}
    assert any(c["off"] for c in cases) and {c["b"] for c in cases} == {1, 2, BC.B, BC.LONG_B}
    assert {c["zero"] for c in cases} == {None, "self", "dup"} and sum(c["bad"] for c in cases) >= 2
    kernels = BC.NO_M05 if (rung, dtype) == ("F", "float32") else BC.KERNELS
    assert {c["kernel"] for c in cases} == set(kernels)
    for c in cases:
        assert (c["metric"] == "F2") <= (c["kernel"] in ("rbf", "matern05")) and (c["kernel"] == "rbf") <= (c["metric"] == "F2")
        if c["zero"] == "self":
            assert c["metric"] == "l2"
    long_case = next(c for c in cases if c["b"] == BC.LONG_B)
    assert long_case["k"] == 5 and long_case["expect"].startswith({"F": "mgp::fused_wave_kernel<", "W": "mgp::backward_wave_kernel<",
                                                                    "L": "mgp::backward_kernel<"}[rung])
    # the inputs: batch_idx drawn with replacement (neighbourhoods share rows), zero distances where the case says so
    P = BC.problem(next(c["id"] for c in cases if c["bi"] and c["b"] == BC.B and c["k"] >= 5 and not c["zero"] and not c["own_query"]))
    assert len(np.unique(P.ni)) < P.ni.size and not (P.ni == P.bi[:, None]).any()
    assert any(len(np.unique(BC.problem(c["id"]).bi)) < c["b"] for c in cases if c["bi"] and c["b"] == BC.B)
    Pz = BC.problem(next(c["id"] for c in cases if c["zero"] == "self"))
    assert ((Pz.ni == Pz.bi[:, None]).sum(1) == 1).all()
    Pd = BC.problem(next(c["id"] for c in cases if c["zero"] == "dup"))
    assert (Pd.ni[:, -1] == Pd.ni[:, 0]).all()


# ---- 4. the inputs keep the reference inside the band, and can tell wrong from right ------------------------------------
@pytest.mark.parametrize("cid", [c["id"] for c in BC.CASES if c["dtype"] == "float32" and c["expect"]])
def test_fp32_restatement_stays_inside_half_of_the_band(cid):
    c, P = BC.BY_ID[cid], BC.problem(cid)
    v64, ref = BC.reference(cid)
    v32 = BC.vjp_rows(P, np.float32, v64.rows)
    assert v32.grad_ls.dtype == v32.grad_noise.dtype == v32.g_nn.dtype == np.float32
    got = BC.compared(c, P, v32)
    for what in ref:
        print(f"{cid}: fp32 restatement {what} {BC.band_error(got[what], ref[what]) / BC.RTOL['float32']:.2e} of the band")
    for what in ref:
        assert_close(got[what], ref[what], HALF, f"fp32 restatement: {what}")


def _pad(a, shape):
    out = np.zeros(shape, dtype=a.dtype)
    out[tuple(slice(0, n) for n in a.shape)] = a
    return out


def _applicable(c):
    """The wrong readings that the case's arguments can tell from the right one."""
    out = set()
    if c["noise"] != "scalar":
        out.add("scalar noise where a table or batch layout was passed")
    if c["bi"] and c["b"] > 1 and c["loocv"] != "yk":  # (y^T K^-1 y knows no query row)
        out.add("batch_idx ignored")
    if c["own_query"]:
        out.add("the query row read from the neighbour table")
    if c["k"] >= 2:
        out.add("the last neighbour dropped")
    if c["d"] >= 2 and (c["aniso"] or c["want"] in ("all", "nn")):
        out.add("the last feature dropped")
    if c["R"] >= 2:
        out.add("the last response dropped")
    # (Matern-1/2 is the one kernel whose slope at zero distance is not zero; on a shared table the two ends of the pair
    # are one row, where the two contributions cancel: grad_feat_nn alone shows the neighbour's end)
    if c["zero"] == "self" and c["kernel"] == "matern05" and c["want"] == "nn":
        out.add("the subgradient at zero distance taken as non-zero")
    if c["b"] >= 2 and c["want"] != "nn":
        out.add("two neighbourhoods' grad_noise rows swapped")
    return out


def _mutants(c, P):
    """{what: the compared outputs under a wrong reading of the arguments}, as far as the case can tell them."""
    k, d, R = c["k"], c["d"], c["R"]
    rows = BC.reference(c["id"])[0].rows
    todo = _applicable(c)
    out = {}

    def run(what, Pm=P, shapes=None, **kw):
        if what not in todo:
            return
        v = BC.vjp_rows(Pm, np.float64, rows, **kw)
        if shapes:
            v.grad_ls, v.grad_noise = _pad(v.grad_ls, (len(rows), d if c["aniso"] else 1)), _pad(v.grad_noise, (len(rows), k))
            v.g_q, v.g_nn, v.g_tg = _pad(v.g_q, (len(rows), d)), _pad(v.g_nn, (len(rows), k, d)), _pad(v.g_tg, (len(rows), k, R))
        out[what] = BC.compared(c, P, v, bi=kw.get("bi"))

    def but(**fields):
        return SimpleNamespace(**{**vars(P), **fields})

    run("scalar noise where a table or batch layout was passed", noise_rows=np.full(P.noise_rows.shape, BC.NOISE))
    run("batch_idx ignored", bi=np.arange(P.b))
    run("the query row read from the neighbour table", Xq=P.Xn)
    if k >= 2:
        run("the last neighbour dropped", but(ni=P.ni[:, :k - 1], noise_rows=P.noise_rows[:, :k - 1]), shapes=True)
    if d >= 2:
        run("the last feature dropped", but(Xn=P.Xn[:, :d - 1], Xq=P.Xq[:, :d - 1], ls=P.ls[:d - 1] if c["aniso"] else P.ls), shapes=True)
    if R >= 2:
        run("the last response dropped", but(Y=P.Y[:, :R - 1], gm=None if P.gm is None else P.gm[:, :R - 1]), shapes=True)
    run("the subgradient at zero distance taken as non-zero", subgradient=1.0)
    if "two neighbourhoods' grad_noise rows swapped" in todo:
        ref = BC.reference(c["id"])[1]
        swapped = {key: a.copy() for key, a in ref.items()}
        swapped["gnz"][[0, 1]] = swapped["gnz"][[1, 0]]
        out["two neighbourhoods' grad_noise rows swapped"] = swapped
    assert set(out) == todo
    return out


ALL_MUTANTS = ("scalar noise where a table or batch layout was passed", "batch_idx ignored", "the query row read from the neighbour table",
               "the last neighbour dropped", "the last feature dropped", "the last response dropped",
               "the subgradient at zero distance taken as non-zero", "two neighbourhoods' grad_noise rows swapped")


@pytest.mark.parametrize("cid", [c["id"] for c in MODE_CASES])
def test_inputs_expose_a_wrong_reading(cid):
    c, P = BC.BY_ID[cid], BC.problem(cid)
    ref = BC.reference(cid)[1]
    for what, got in _mutants(c, P).items():
        moved = max(BC.band_error(got[key], ref[key]) for key in ref)
        print(f"{cid}: {what}: {moved / BC.RTOL['float32']:.1f} bands")
        assert moved >= MOVED, (what, moved)


def test_every_mutant_has_a_case_in_every_rung():
    for rung in BC.RUNGS:
        for dtype in ("float32", "float64"):
            seen = set().union(*(_applicable(c) for c in MODE_CASES if c["rung"] == rung and c["dtype"] == dtype))
            # (fp32 F draws no Matern-1/2: the Gram form of its prepared shapes serves the other four)
            missing = set(ALL_MUTANTS) - seen
            assert missing <= ({"the subgradient at zero distance taken as non-zero"} if (rung, dtype) == ("F", "float32") else set()), (rung, dtype, missing)
