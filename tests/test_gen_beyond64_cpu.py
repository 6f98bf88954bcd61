"""CPU: the general-smoothness Matern beyond 64 slots (mgp_posterior_gen_*, mgp_posterior_gen_generic_*,
mgp_posterior_gen_large_*, mgp_max_nn_count_gen; include/muygpys_hip.h) -- the status of every refused or empty call,
decided BEFORE any HIP call, the limit against the LDS arithmetic, what muygpys_amd.fused hands the entries and in which
order it tries them, and the compiler's register record of the four general-smoothness instantiations.

Status rows: one rule is violated per row, starting from arguments that would launch; host buffers stand in for device
pointers (nothing dereferences them before the status is decided).  No row here reaches a launch."""

import ctypes as C
import json
import os

import pytest
import torch

from muygpys_amd import _lib, fused
from muygpys_amd.fused import FusedUnsupported, KernelSpec
from tests.call_recorder import STREAM, install, vals

OK, EINVAL, EUNSUPPORTED = 0, -1, -2
ES = {"f32": 4, "f64": 8}
INT_MAX, INT64_MAX = 2**31 - 1, 2**63 - 1
NAN = float("nan")

ENTRIES = {
    "posterior_gen": "fq fn pq qs pn ns d bi ni b k tg R tb nm eps nd nu mid ls lsc mean var yk info st",
    "posterior_gen_generic": "fq fn d bi ni b k tg R tb nm eps nd nu mid ls lsc mean var yk info st",
    "posterior_gen_large": "fq fn d bi ni b k tg R tb nm eps nd nu mid ls lsc mean var yk info ws wsb st",
}
NUMBERS = dict(qs=0, ns=0, d=4, b=3, k=5, R=1, tb=0, nm=0, eps=1e-3, nu=0.8, mid=0, lsc=1, wsb=1 << 40)
OPTIONAL = ("nd", "st", "pq", "pn")
REQUIRED = "fq fn tg ni ls mean var"
BUF = (C.c_double * 64)()
PTR = C.addressof(BUF)
assert PTR % 16 == 0


def status(entry, suf, **changes):
    names = ENTRIES[entry].split()
    args = {n: NUMBERS[n] if n in NUMBERS else (None if n in OPTIONAL else PTR) for n in names}
    unknown = set(changes) - set(names)
    assert not unknown, (entry, unknown)
    args.update(changes)
    return getattr(_lib.load(), f"mgp_{entry}_{suf}")(*[args[n] for n in names])


def max_gen(es, R=1):
    return _lib.load().mgp_max_nn_count_gen(es, R)


def rows_of(entry, es):
    """(name, changes, status): every rung of the check order.  Rows that pass every check stop at "does not fit LDS" or
    "more than 1024 rows", so none launches."""
    names = ENTRIES[entry].split()
    large, named = entry == "posterior_gen_large", entry != "posterior_gen"
    nofit = max_gen(es) + 1  # (the LDS kernel refuses; the slab kernel would launch: never without its own refusal below)
    stop = dict(k=1023) if large else dict(k=nofit)
    # 1. sizes and the smoothness, in front of everything
    rows = [("b < 0", dict(b=-1), EINVAL), ("k < 1", dict(k=0), EINVAL), ("d < 1", dict(d=0), EINVAL), ("R < 1", dict(R=0), EINVAL)]
    rows += [(f"smoothness {v}", dict(nu=v), EINVAL) for v in (0.0, -1.5, NAN)]
    nothing = {n: None for n in names if n not in NUMBERS}
    rows.append(("smoothness NaN, empty batch", dict(nu=NAN, b=0, **nothing), EINVAL))
    # 2. the empty batch
    rows.append(("empty batch, all pointers NULL", dict(b=0, **nothing, **({"wsb": 0} if large else {})), OK))
    rows.append(("empty batch, ids and smoothness 31 not looked at", dict(b=0, **nothing, nu=31.0, mid=7, nm=8, lsc=9), OK))
    rows.append(("empty batch, k < 1", dict(b=0, k=0), EINVAL))
    # 3. pointers, ids, workspace -- also where a later rung would refuse
    for extra, tag in ((dict(), ""), (dict(nu=31.0), ", smoothness 31"), (stop, ", a system nothing serves")):
        rows += [(f"{p} NULL{tag}", {p: None, **extra}, EINVAL) for p in REQUIRED.split()]
        rows += [(f"metric id {i}{tag}", dict(mid=i, **extra), EINVAL) for i in (-1, 2)]
        rows += [(f"noise mode {i}{tag}", dict(nm=i, **extra), EINVAL) for i in (-1, 3)]
        rows += [(f"noise mode {i} without noise_dev{tag}", dict(nm=i, nd=None, **extra), EINVAL) for i in (1, 2)]
        rows += [(f"ls_count {i} at d = 4{tag}", dict(lsc=i, **extra), EINVAL) for i in (0, 2, 5)]
        if large:
            rows.append((f"workspace NULL{tag}", dict(ws=None, **extra), EINVAL))
            rows.append((f"workspace misaligned{tag}", dict(ws=PTR + 8, **extra), EINVAL))
            rows.append((f"workspace of 15 bytes{tag}", dict(wsb=15, **extra), EINVAL))
    # 4. what the kernels do not serve
    rows.append(("smoothness 30.5", dict(nu=30.5), EUNSUPPORTED))
    rows.append(("smoothness inf", dict(nu=float("inf")), EUNSUPPORTED))
    rows.append(("k + 1 + R = 1025", dict(k=1023), EUNSUPPORTED))
    rows.append(("k + 1 + R = 1025 by responses", dict(k=1008, R=16), EUNSUPPORTED))
    big = dict(wsb=INT64_MAX) if large else {}
    rows.append(("k = INT_MAX", dict(k=INT_MAX, **big), EUNSUPPORTED))
    rows.append(("k = R = INT_MAX", dict(k=INT_MAX, R=INT_MAX, **big), EUNSUPPORTED))
    if large:
        rows.append(("k = INT_MAX, a workspace of 1 TiB", dict(k=INT_MAX), EINVAL))
    else:
        rows.append(("one beyond mgp_max_nn_count_gen", dict(k=nofit), EUNSUPPORTED))
        rows.append(("... with 16 responses", dict(k=max_gen(es, 16) + 1, R=16), EUNSUPPORTED))
        rows.append(("... and d = 70", dict(k=nofit, d=70, lsc=70), EUNSUPPORTED))
    if not named:
        # prepared tables beyond 64 slots stay refused (a 64-byte stride covers d = 4 and the response slot)
        rows.append(("prepared tables, 65 slots", dict(fq=None, fn=None, pq=PTR, qs=64, pn=PTR, ns=64, k=63), EUNSUPPORTED))
        rows.append(("prepared tables, 1025 rows", dict(fq=None, fn=None, pq=PTR, qs=64, pn=PTR, ns=64, k=1023), EUNSUPPORTED))
    return rows


GRID = [(e, s, n, ch, want) for e in ENTRIES for s in ES for n, ch, want in rows_of(e, ES[s])]


@pytest.mark.parametrize("entry, suf, name, changes, want", GRID, ids=[f"{e}_{s}: {n}" for e, s, n, _, _ in GRID])
def test_status_of_refused_and_empty_calls(entry, suf, name, changes, want):
    assert status(entry, suf, **changes) == want


@pytest.mark.parametrize("suf", ["f32", "f64"])
def test_workspace_one_byte_short_of_a_slab(suf):
    lib, es = _lib.load(), ES[suf]
    for k, R in ((5, 1), (200, 1), (1022, 1), (1007, 16)):
        assert status("posterior_gen_large", suf, k=k, R=R, wsb=lib.mgp_large_workspace_bytes(es, k, R, 1) - 1) == EINVAL, (k, R)


def test_closed_form_entries_keep_their_treatment_of_the_general_id():
    """mgp_posterior_large_*: MGP_EUNSUPPORTED; mgp_posterior_generic_*: MGP_EINVAL (they have no smoothness argument)."""
    lib = _lib.load()
    for suf in ES:
        head = [PTR, PTR, 4, PTR, PTR, 3, 5, PTR, 1]
        tail = [0, 1e-3, None, 5, 0, PTR, 1, PTR, PTR, PTR, PTR]
        assert getattr(lib, f"mgp_posterior_generic_{suf}")(*head, *tail, None) == EINVAL
        assert getattr(lib, f"mgp_posterior_large_{suf}")(*head, 0, *tail, PTR, 1 << 40, None) == EUNSUPPORTED


def test_limit_against_the_lds_arithmetic():
    """mgp_max_nn_count_gen: the LDS rule of mgp_max_nn_count -- index slots, the (k + 1 + R) rows of the system at their
    padded stride, a (k + 1) x 8 feature tile with its pad, 8 scale slots, k pivots, a flag, in 160 KiB -- with the node
    table behind it: 2 x 128 floats or 2 x 256 doubles."""
    lib = _lib.load()

    def lds_bytes(es, k, R, dc=8):
        e = 16 // es
        stride = (((k + 1 + e - 1) // e) | 1) * e  # rows of k + 1 elements in whole 16-byte slots, an odd number of them
        n = ((k + 2) & ~1) * 8 + ((k + 1 + R) * stride + (k + 1) * (dc + e) + dc + k) * es + 16
        return (n + 15) & ~15

    for es, table in ((4, 2 * 128 * 4), (8, 2 * 256 * 8)):
        for R in (1, 3, 16):
            kc, kg = lib.mgp_max_nn_count(es, R), lib.mgp_max_nn_count_gen(es, R)
            assert lds_bytes(es, kc, R) <= 160 * 1024 < lds_bytes(es, kc + 1, R), (es, R, kc)  # (the rule is the library's)
            assert lds_bytes(es, kg, R) + table <= 160 * 1024 < lds_bytes(es, kg + 1, R) + table, (es, R, kg)
            assert 0 < kc - kg <= 3, (es, R, kc, kg)  # below by what the table costs: a row or two of the system
            assert kg >= 65
    assert lib.mgp_max_nn_count_gen(4, 1) < lib.mgp_max_nn_count(4, 1) and lib.mgp_max_nn_count_gen(8, 1) < lib.mgp_max_nn_count(8, 1)
    assert lib.mgp_max_nn_count_gen(2, 1) == -1 and lib.mgp_max_nn_count_gen(0, 1) == -1


# ---- what muygpys_amd.fused hands the entries ------------------------------------------------------------------------
K, D, R, B, N, NQ = 70, 3, 2, 7, 200, 9
F32 = torch.float32


@pytest.fixture
def rec(monkeypatch):
    yield install(monkeypatch)
    fused.clear_caches()


def tables(k=K, seed=0):
    g = torch.Generator().manual_seed(seed)
    X = torch.randn(N, D, generator=g)
    Xq = torch.randn(NQ, D, generator=g)
    Y = torch.randn(N, R, generator=g)
    bi = torch.randint(0, NQ, (B,), generator=g)
    ni = torch.randint(0, N, (B, k), generator=g)
    return X, Xq, Y, bi, ni


SPEC = KernelSpec("matern_gen", "l2", (2.0, 3.0, 4.0), 1e-3, smoothness=0.42)


@pytest.mark.parametrize("gathered", [False, True])
@pytest.mark.parametrize("packed", [False, True, "auto"])
def test_auto_beyond_64_slots_is_one_call_on_the_plain_tables(rec, packed, gathered):
    X, Xq, Y, bi, ni = tables()
    tg = Y[ni] if gathered else Y
    mean, var, yk = fused.posterior_mean_var(SPEC, Xq, X, bi, ni, tg, want_ykinvy=True, packed=packed, gathered=gathered)
    assert [c[0] for c in rec.calls] == ["posterior_gen"]  # no table_pack, no prepared tables, whatever `packed` says
    v = vals(rec.calls[0])
    # fq, fn, packed_q, q_stride, packed_nn, nn_stride, d, bi, ni, b, k, tg, R, targets_batch, noise_mode, eps, nd,
    # smoothness, metric, ls, ls_count, mean, var, ykinvy, info, stream
    assert len(v) == 26 and rec.calls[0][1] == F32
    assert v[0:6] == [Xq.data_ptr(), X.data_ptr(), None, 0, None, 0]
    assert v[6:17] == [D, bi.data_ptr(), ni.data_ptr(), B, K, tg.data_ptr(), R, int(gathered), 0, 1e-3, None]
    assert v[17:19] == [0.42, 0] and v[19] is not None and v[20] == D
    assert v[21:] == [mean.data_ptr(), var.data_ptr(), yk.data_ptr(), None, STREAM]


@pytest.mark.parametrize("gathered", [False, True])
def test_the_generic_family_by_name(rec, gathered):
    X, Xq, Y, bi, ni = tables()
    tg = Y[ni] if gathered else Y
    info = torch.zeros(1, dtype=torch.int32)
    mean, var = fused.posterior_mean_var(SPEC, Xq, X, bi, ni, tg, path="generic", gathered=gathered, info=info)
    (call,) = rec.calls
    v = vals(call)
    # fq, fn, d, bi, ni, b, k, tg, R, targets_batch, noise_mode, eps, nd, smoothness, metric, ls, ls_count, mean, var,
    # ykinvy, info, stream
    assert call[0] == "posterior_gen_generic" and len(v) == 22
    assert v[0:13] == [Xq.data_ptr(), X.data_ptr(), D, bi.data_ptr(), ni.data_ptr(), B, K, tg.data_ptr(), R, int(gathered), 0, 1e-3, None]
    assert v[13:15] == [0.42, 0] and v[15] is not None and v[16] == D
    assert v[17:] == [mean.data_ptr(), var.data_ptr(), None, info.data_ptr(), STREAM]


@pytest.mark.parametrize("k", [5, K])
def test_the_large_family_by_name(rec, k):
    X, Xq, Y, bi, ni = tables(k)
    mean, var, yk = fused.posterior_mean_var(SPEC, Xq, X, None, ni, Y, path="large", want_ykinvy=True)
    (call,) = rec.calls
    v = vals(call)
    # ... ykinvy, info, workspace, workspace_bytes, stream
    assert call[0] == "posterior_gen_large" and len(v) == 24
    assert v[0:13] == [Xq.data_ptr(), X.data_ptr(), D, None, ni.data_ptr(), B, k, Y.data_ptr(), R, 0, 0, 1e-3, None]
    assert v[13:15] == [0.42, 0] and v[15] is not None and v[16] == D
    assert v[17:21] == [mean.data_ptr(), var.data_ptr(), yk.data_ptr(), None]
    assert v[21] is not None and v[21] % 16 == 0 and v[22] == _lib.load().mgp_large_workspace_bytes(4, k, R, B) and v[23] == STREAM


def test_a_refusal_of_the_lds_kernel_is_followed_by_exactly_one_slab_call(rec):
    X, Xq, Y, bi, ni = tables()
    rec.statuses["posterior_gen"] = [-2]
    mean, var = fused.posterior_mean_var(SPEC, Xq, X, bi, ni, Y)
    assert [c[0] for c in rec.calls] == ["posterior_gen", "posterior_gen_large"]
    first, second = (vals(c) for c in rec.calls)
    assert second[0:13] == first[0:2] + first[6:17] and second[13:17] == first[17:21]  # the same tables, shape, noise, model
    assert second[17:21] == first[21:25] == [mean.data_ptr(), var.data_ptr(), None, None] and second[23] == STREAM


def test_a_refusal_of_both_is_fused_unsupported(rec):
    X, Xq, Y, bi, ni = tables()
    rec.statuses["posterior_gen"] = [-2]
    rec.statuses["posterior_gen_large"] = [-2]
    with pytest.raises(FusedUnsupported, match="general-smoothness Matern: no fused kernel"):
        fused.posterior_mean_var(SPEC, Xq, X, bi, ni, Y)
    assert [c[0] for c in rec.calls] == ["posterior_gen", "posterior_gen_large"]


def test_more_than_1024_rows_is_fused_unsupported_without_a_slab_call(rec):
    X, Xq, Y, bi, _ = tables()
    ni = torch.randint(0, N, (B, 1022))  # with two responses: 1025 rows
    rec.statuses["posterior_gen"] = [-2]
    with pytest.raises(FusedUnsupported):
        fused.posterior_mean_var(SPEC, Xq, X, bi, ni, Y)
    assert [c[0] for c in rec.calls] == ["posterior_gen"]


@pytest.mark.parametrize("packed", [False, True])
def test_up_to_64_slots_a_refusal_still_makes_one_call_and_raises(rec, packed):
    X, Xq, Y, bi, ni = tables(5)
    rec.statuses["posterior_gen"] = [-2]
    with pytest.raises(FusedUnsupported, match="general-smoothness Matern: no fused kernel"):
        fused.posterior_mean_var(SPEC, Xq, X, bi, ni, Y, packed=packed)
    assert [c[0] for c in rec.calls if c[0] != "table_pack"] == ["posterior_gen"]
    # ... and 64 slots exactly are still the wave kernels' alone: k + 1 + R = 64
    rec.calls.clear()
    rec.statuses["posterior_gen"] = [-2]
    with pytest.raises(FusedUnsupported):
        fused.posterior_mean_var(SPEC, Xq, X, bi, torch.randint(0, N, (B, 61)), Y, packed=False)
    assert [c[0] for c in rec.calls] == ["posterior_gen"]


def test_named_paths_refuse_what_they_refused(rec):
    X, Xq, Y, bi, ni = tables()
    with pytest.raises(ValueError, match=r"the general-smoothness Matern goes through the dispatcher \(path='auto'\)"):
        fused.posterior_mean_var(SPEC, Xq, X, bi, ni, Y, path="rhs")
    with pytest.raises(ValueError, match="gathered responses go through the dispatcher"):
        fused.posterior_mean_var(KernelSpec("matern15", "l2", 2.0, 1e-3), Xq, X, bi, ni, Y[ni], path="generic", gathered=True)
    assert rec.calls == []
    rec.statuses["posterior_gen_generic"] = [-2]
    with pytest.raises(FusedUnsupported):
        fused.posterior_mean_var(SPEC, Xq, X, bi, ni, Y, path="generic")
    assert [c[0] for c in rec.calls] == ["posterior_gen_generic"]  # a named family is not followed by another


# ---- the compiler's record -------------------------------------------------------------------------------------------
def test_general_instantiations_no_spills_no_scratch():
    path = os.path.join(os.path.dirname(_lib.LIB_PATH), "kernel_resources.json")
    with open(path) as f:
        res = json.load(f)
    mine = {n: r for n, r in res.items() if "fused_generic_gen_kernel" in n or "fused_large_gen_kernel" in n}
    assert len(mine) == 4, sorted(mine)  # two families, two float widths
    for name, r in mine.items():
        assert r["VGPRs Spill"] == 0, (name, r)
        assert r["ScratchSize [bytes/lane]"] == 0, (name, r)
    # the closed-form instantiations of the LDS family are in the record now, under the names they had
    closed = [n for n in res if "fused_generic_kernel" in n]
    assert len(closed) == 2 and all(res[n]["VGPRs Spill"] == 0 and res[n]["ScratchSize [bytes/lane]"] == 0 for n in closed), closed
