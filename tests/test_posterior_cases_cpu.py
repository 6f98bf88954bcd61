"""What tests/test_gpu_posterior_modes.py relies on, asserted with the numpy oracle alone (no GPU): the sample of
tests/posterior_cases.py covers every value of every argument mode in every kernel family and the shapes each entry
of the family table names, its restatement is the oracle's, plain fp32 arithmetic stays inside a quarter of the
project's fp32 band on every case, and every wrong reading of a mode -- noise rows reversed, taken from the next
neighbourhood or through a wrong table index, the query row of the next neighbourhood, the response rows reversed --
moves the outputs of every case far outside that band."""

import numpy as np
import pytest

from oracle import muygps_oracle as orc
from tests import posterior_cases as PC
from tests.util import RTOL, assert_close, assert_rel_close

QUARTER = RTOL["float32"] / 4   # what plain fp32 arithmetic may cost on these inputs
MOVED = 10 * RTOL["float32"]    # what a wrong mode must cost ...
SHARE = 0.10                    # ... in this share of the neighbourhoods
IDS = [c["id"] for c in PC.CASES]
ENTRY_IDS = [c["id"] for c in PC.ENTRY_CASES]


def _entry_cases(name, dtype):
    return [c for c in PC.CASES if c["entry"] == name and c["dtype"] == dtype and c["b"] == PC.B]


def test_every_family_sees_every_factor_value():
    assert len(PC.FAMILIES) == 11
    for family in PC.FAMILIES:
        cases = [c for c in PC.CASES if c["family"] == family]
        seen = {name: {c[name] for c in cases} for name in ("noise", "gathered", "bi", "own_query", "aniso", "kernel", "metric")}
        assert seen["noise"] == {"scalar", "table", "batch"}, family
        for name in ("gathered", "bi", "own_query", "aniso"):
            assert seen[name] == {False, True}, (family, name)
        served = set(PC.NO_M05 if family.startswith("rhs_mf") else PC.KERNELS)
        assert seen["kernel"] == served and seen["metric"] == {"l2", "F2"}, (family, seen)
        small = [c for c in cases if c["b"] != PC.B]
        assert len(small) == 2 and all(c["b"] in (1, 2, 3) and c["noise"] == "batch" and c["gathered"] and not c["bi"] for c in small)
    for e in PC.ENTRIES:
        assert len(_entry_cases(e["name"], e["dtype"])) in (5, 6), e["name"]
    for c in PC.CASES:  # kernel and metric are paired as far as the pair is a covariance function
        assert (c["metric"] == "F2") <= (c["kernel"] in ("rbf", "matern05")) and (c["kernel"] == "rbf") <= (c["metric"] == "F2")
    assert {c["family"] for c in PC.LONG_CASES} == set(PC.FAMILIES) and len(PC.LONG_CASES) == len(PC.FAMILIES)
    for c in PC.LONG_CASES:
        assert c["b"] == PC.LONG_B < 65536 and c["noise"] == "batch" and c["gathered"] and not c["bi"]
        assert c["R"] <= (5 if c["family"].startswith("rhs_mf") else 3)


def test_entries_name_the_shapes_of_the_issue():
    def shapes(name, dtype):
        return {(c["k"], c["R"], c["d"], c["off"]) for c in _entry_cases(name, dtype)}

    for dtype in ("float32", "float64"):
        f32 = dtype == "float32"
        assert {(30, 1, 8, False), (20, 3, 12, False)} <= shapes("W32p", dtype)          # a full and a padded tile
        assert {(20, 3, 3, False), (25, 1, 70, False), (30, 1, 8, True)} <= shapes("W32r", dtype)
        assert {(62, 1, 8, False), (47, 16, 16, False)} <= shapes("W64p", dtype)          # 64 rows, two ways
        assert {d for _, _, d, _ in shapes("W64r", dtype)} >= {6 if f32 else 7, 72}
        assert any(d % (4 if f32 else 2) for pk in ("W32pk", "W64pk") for _, _, d, _ in shapes(pk, dtype))  # a padded prepared row
        assert shapes("S30", dtype) == shapes("S30pk", dtype) == {(30, 1, 40, False)}
        assert shapes("S50", dtype) == shapes("S50pk", dtype) == {(50, 1, 8, False)}
        wide = "WIDE" if f32 else "WIDE64"
        rows = {name: {k + 1 + R for k, R, _, _ in shapes(name, dtype)} for name in (f"{wide}_{17 if f32 else 18}", f"{wide}_24", f"{wide}_32")}
        assert 67 in rows[f"{wide}_{17 if f32 else 18}"] and 93 in rows[f"{wide}_24"] and {122, 128} <= rows[f"{wide}_32"]
        for name in rows:
            assert {3, 64} <= {d for _, _, d, _ in shapes(name, dtype)}, name
        gen = {(c["k"], c["R"], c["d"], c["path"]) for c in _entry_cases("GEN", dtype)}
        assert {(12, 3, 3, "generic"), (70, 1, 70, "auto"), (70, 17, 8, "auto")} <= gen
    auto = {(c["entry"], c["k"], c["R"]) for c in PC.CASES if c["path"] == "auto"}
    assert ("RHS4g", 64, 3) in auto and ("RHS16f", 60, 16) in auto
    mf = {(c["k"], c["d"]) for c in _entry_cases("MF", "float32")}
    assert any(k == 64 for k, _ in mf) and any(d == 64 for _, d in mf)
    assert {c["d"] for c in _entry_cases("RHS16fold", "float32")} == {44, 48}
    assert all(c["off"] for c in _entry_cases("RHS16w3", "float32"))


@pytest.mark.parametrize("cid", IDS + ENTRY_IDS + [c["id"] for c in PC.LONG_CASES])
def test_shape_constraints_of_the_entry(cid):
    """The conditions under which the dispatch code (csrc/mgp_fused_wave.hip, mgp_fused_rhs.hip, mgp_fused_rhs_mf.hip,
    mgp_fused_wide.hip, mgp_fused_wide64.hip, mgp_capi.hip: posterior) reaches the kernel the entry names."""
    c = PC.BY_ID[cid]
    k, R, d, rows = c["k"], c["R"], c["d"], PC.rows_of(c)
    es = 4 if c["dtype"] == "float32" else 8
    E, entry = 16 // es, c["entry"]
    m05 = c["kernel"] == "matern05"
    assert c["path"] in ("auto", "rhs", "generic") and (c["path"] == "auto" or not (c["gathered"] or c["packed"]))
    assert (k, R, d) not in ((30, 1, 40), (50, 1, 8)) or entry.startswith("S")
    if c["packed"]:
        import torch

        from muygpys_amd.fused import PackedTable

        t = torch.float32 if es == 4 else torch.float64
        assert PackedTable.supported(d, 0, k + R, t) if c["gathered"] else PackedTable.supported(d, R, k, t), cid
        assert not c["off"] and (not c.get("can_gather") or PackedTable.supported(d, 0, k + R, t))
        d =(d + E - 1) // E * E  # (the kernels see the prepared row, padded to whole 16-byte groups)
    one_stage = (d + 2 * E - 1) // (2 * E) * (2 * E) <= 64
    if entry[0] in "WS" and not entry.startswith("WIDE"):
        assert rows <= 32 if "32" in entry or entry.startswith("S30") else 32 < rows <= 64
        piped = d % E == 0 and one_stage and not c["off"]
        assert piped == (not entry.endswith("r")) or c["packed"]
        assert not c["packed"] or c["gathered"] or R <= E
    elif c["family"].startswith("rhs"):
        assert k <= 64 and R <= 16 and (c["path"] == "rhs" or rows > 64 or c["packed"])
        gram = es == 4 and one_stage and d % E == 0 and d >= 2 * E and not m05
        dpad = (d + 7) // 8 * 8
        mf = es == 4 and 4 < R and not c["yk"] and gram and not c["off"] and not (dpad == 48 and c["b"] >= 2)
        assert mf == entry.startswith("MF")
        if entry.startswith("RHS4"):
            assert R <= 4 and (es == 8 or gram == (entry == "RHS4g"))
        else:
            assert 4 < R
            assert c["yk"] == (entry == "RHS16f")
            if es == 4 and not c["yk"] and not mf:
                fold = gram and not c["off"] and c["b"] >= 2 and dpad <= 48
                assert {"RHS16fold": gram and fold, "RHS16w3": gram and not fold, "RHS16b": not gram}[entry]
    elif c["family"].startswith("wide"):
        assert k >= 65 and 65 <= rows <= 128 and R <= 16 and d <= 64
        ng = next(n for n, top in (((17 if es == 4 else 18), (68 if es == 4 else 72)), (20, 80), (22, 88), (24, 96), (26, 104), (28, 112),
                                   (30, 120), (32, 128)) if rows <= top)
        assert entry.endswith(f"_{ng}")
    else:
        assert entry == "GEN" and (c["path"] == "generic" or (rows > 64 and k > 64 and (d > 64 or R > 16)))


def test_restatement_is_the_oracle():
    """outputs(case, float64) against oracle.muygps_oracle, assembled as tests/test_gpu_large.py::oracle_outputs does."""
    for c in PC.CASES[::7]:
        P = PC.problem(c["id"])
        ospec = orc.Spec(c["kernel"], c["metric"], P.ls, 0.0)
        Kc, Kin = orc.kernel_tensors(ospec, orc.crosswise_tensor(P.Xq, P.Xn, P.bi, P.ni), orc.pairwise_tensor(P.Xn, P.ni))
        Kin = Kin + np.stack([np.diag(r) for r in P.noise_rows])
        Yn = P.Y[P.ni]
        A = np.linalg.solve(Kin, np.concatenate([Kc[:, :, None], Yn], axis=2))
        ref = (np.einsum("bk,bkr->br", Kc, A[:, :, 1:]), 1.0 - np.einsum("bk,bk->b", Kc, A[:, :, 0]),
               np.einsum("bkr,bkr->br", Yn, A[:, :, 1:]))
        for got, want, what in zip(PC.reference(c["id"]), ref, ("mean", "var", "ykinvy")):
            assert_close(got, want, 1e-10, f"{c['id']}: {what}")
        if c["noise"] != "scalar":
            assert np.array_equal(P.noise_rows, P.table[P.ni])


def _moved(c, ref, mean, var):
    """The share of the neighbourhoods whose mean (in the assert_close form) or variance (relative) left by more than
    MOVED.  ``var`` None: the mean alone."""
    m_ref, v_ref, _ = ref
    rms = float(np.sqrt(np.mean(m_ref**2)))
    out = (np.abs(mean - m_ref) > MOVED * (np.abs(m_ref) + rms)).any(axis=1)
    if var is not None:
        out |= np.abs(var - v_ref) > MOVED * np.abs(v_ref)
    return out.mean()


@pytest.mark.parametrize("cid", IDS + ENTRY_IDS)
def test_inputs_allow_the_band_and_expose_a_wrong_mode(cid):
    c = PC.BY_ID[cid]
    P = PC.problem(cid)
    ref = PC.reference(cid)
    # plain fp32 arithmetic: a quarter of the band
    m32, v32, y32 = PC.outputs(c, np.float32)
    assert m32.dtype == v32.dtype == y32.dtype == np.float32
    print(f"{cid}: fp32 restatement mean {PC.band_error(m32, ref[0]):.2e} var {PC.rel_error(v32, ref[1]):.2e} "
          f"ykinvy {PC.rel_error(y32, ref[2]):.2e}")
    assert_close(m32, ref[0], QUARTER, "fp32 restatement: mean")
    assert_rel_close(v32, ref[1], QUARTER, "fp32 restatement: var")
    assert_rel_close(y32, ref[2], QUARTER, "fp32 restatement: ykinvy")
    assert np.all(ref[1] > 0) and np.all(ref[2] > 0)
    # the mutations, in fp64 on the pieces of the reference
    Kin, Kc = PC.covariances(c, P, np.float64)
    Yn = P.Y[P.ni]
    nz = P.noise_rows
    muts = {}
    if c["noise"] != "scalar":
        muts["noise rows reversed"] = PC.solve(Kin, Kc, nz[:, ::-1], Yn)[:2]
    if c["noise"] == "batch" and c["b"] > 1:
        muts["noise rows of the next neighbourhood"] = PC.solve(Kin, Kc, np.roll(nz, -1, axis=0), Yn)[:2]
    if c["noise"] == "table":
        muts["noise table through a wrong index"] = PC.solve(Kin, Kc, P.table[(P.ni + 1) % PC.N], Yn)[:2]
    if c["b"] > 1:
        muts["query row of the next neighbourhood"] = PC.solve(Kin, PC.covariances(c, P, np.float64, bi=np.roll(P.bi, -1))[1], nz, Yn)[:2]
    muts["response rows reversed"] = (PC.solve(Kin, Kc, nz, Yn[:, ::-1])[0], None)
    for what, (mean, var) in muts.items():
        share = _moved(c, ref, mean, var)
        print(f"{cid}: {what}: {share:.2f} of the neighbourhoods moved")
        assert share >= SHARE, (what, share)
