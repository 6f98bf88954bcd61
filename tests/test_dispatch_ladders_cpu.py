"""CPU: the fallback ladder of every fused Python function -- which entry points it tries, in which order, with which
arguments, and how the end status comes back.

A ladder: try an entry point; on ``MGP_EUNSUPPORTED`` (-2) try the next; a slab entry (``*_large_*``) gets a workspace
sized by the library's ``*_workspace_bytes`` query first.  ``_lib.fn`` is the recorder of tests/call_recorder.py, so
every call stops at the library boundary and answers with the status queued for it.  Each test checks the sequence of
entry points, that a later rung is handed what the first one was (tables, shape, noise, model, outputs), the workspace
pointer and byte count at the positions include/muygpys_hip.h gives them, and the outcome: the value returned or the
exception with its message.

Shapes: those of test_fused_calls_cpu.py (fp32, k = 5, d = 3, b = 7); the general smoothness beyond 64 slots: k = 70.
The coefficient ladder (``mgp_fast_coefficients_*`` -> ``_any_*`` -> None) is pinned by test_fast_any_cpu.py."""

import pytest
import torch

from muygpys_amd import _lib, autograd, fused
from muygpys_amd._src.gp.muygps import hip as M
from muygpys_amd.fused import FusedUnsupported, KernelSpec
from tests.call_recorder import STREAM, install, vals

K, D, R, B, N, NQ = 5, 3, 2, 7, 40, 9
UNSUPPORTED, EINVAL = -2, -1
# (workspace, workspace_bytes, stream) close every slab entry; position of `workspace` / argument count
WORKSPACE_AT = {"posterior_large": (21, 24), "posterior_gen_large": (21, 24), "hyper_backward_large": (21, 24),
                "solve_large": (12, 15)}


@pytest.fixture
def rec(monkeypatch):
    yield install(monkeypatch)
    fused.clear_caches()


@pytest.fixture
def resets(monkeypatch):
    seen = []
    monkeypatch.setattr(_lib, "loocv_scratch_reset", lambda: seen.append(1))
    return seen


def tables(k=K, one_response=False, seed=0):
    g = torch.Generator().manual_seed(seed)
    X = torch.randn(N, D, generator=g)
    Xq = torch.randn(NQ, D, generator=g)
    Y = torch.randn(N, generator=g) if one_response else torch.randn(N, R, generator=g)
    bi = torch.randint(0, NQ, (B,), generator=g)
    ni = torch.randint(0, N, (B, k), generator=g)
    return X, Xq, Y, bi, ni


def spec_of(kernel="matern15", noise=1e-3):
    return KernelSpec(kernel, "l2", (2.0, 3.0, 4.0), noise, smoothness=0.42 if kernel == "matern_gen" else None)


def names(rec, *skip):
    return [c[0] for c in rec.of(*skip)]


def large_bytes(k, R, b=B):
    return _lib.load().mgp_large_workspace_bytes(4, k, R, b)


def check_workspace(call, want_bytes):
    at, count = WORKSPACE_AT[call[0]]
    v = vals(call)
    assert len(v) == count and want_bytes > 0
    assert v[at] is not None and v[at + 1] == want_bytes and v[at + 2] == STREAM


def queue(rec, **statuses):
    for base, status in statuses.items():
        rec.statuses[base] = [status]


def rows_message(k, R):
    return (rf"nn_count = {k} with {R} response column\(s\) exceeds mgp_large_max_nn_count = "
            rf"{_lib.load().mgp_large_max_nn_count(4, R)} \(a local system holds at most 1024 rows: nn_count \+ 1 \+ response_count\)")


# ---- posterior_mean_var, closed-form kernel ---------------------------------------------------------------------------

def closed_form_rungs(packed, gathered):
    plain = "posterior_gathered" if gathered else "posterior"
    return (["posterior_packed_gathered" if gathered else "posterior_packed"] if packed else []) + [plain, "posterior_large"]


def check_plain_then_large(plain, large, gathered):
    """mgp_posterior[_gathered]_*: fq fn d bi ni b k tg R | noise(3) kernel metric ls ls_count mean var ykinvy info | stream;
    mgp_posterior_large_* has targets_batch behind R and (workspace, workspace_bytes) in front of the stream."""
    p, v = vals(plain), vals(large)
    assert len(p) == 21 and v[0:9] == p[0:9] and v[9] == int(gathered) and v[10:21] == p[9:20]


@pytest.mark.parametrize("gathered", [False, True])
@pytest.mark.parametrize("packed", [False, True])
def test_closed_form_auto_prepared_plain_slab(rec, packed, gathered):
    X, Xq, Y, bi, ni = tables()
    tg = Y[ni] if gathered else Y
    rungs = closed_form_rungs(packed, gathered)
    queue(rec, **{base: UNSUPPORTED for base in rungs[:-1]})
    mean, var, yk = fused.posterior_mean_var(spec_of(), Xq, X, bi, ni, tg, want_ykinvy=True, packed=packed, gathered=gathered)
    assert names(rec) == rungs
    assert mean.shape == (B, R) and var.shape == (B,) and yk.shape == (B, R)
    plain, large = rec.of()[-2:]
    assert vals(plain)[0:9] == [Xq.data_ptr(), X.data_ptr(), D, bi.data_ptr(), ni.data_ptr(), B, K, tg.data_ptr(), R]
    check_plain_then_large(plain, large, gathered)
    check_workspace(large, large_bytes(K, R))
    if packed:
        # packed_q q_stride packed_nn nn_stride d bi ni b k ...: the same neighbourhoods and outputs, d_kernel = 4 features
        first = vals(rec.of()[0])
        assert first[4:9] == [4] + vals(plain)[3:7] and first[-5:] == vals(plain)[-5:]
    assert vals(large)[17:21] == [mean.data_ptr(), var.data_ptr(), yk.data_ptr(), None]


@pytest.mark.parametrize("status, text", [(EINVAL, "MGP_EINVAL"), (_lib.EHIP - 5, "HIP runtime error 5")])
@pytest.mark.parametrize("failing", [0, 1, 2])
def test_closed_form_auto_ends_at_any_other_status_and_is_named_mgp_posterior(rec, failing, status, text):
    X, Xq, Y, bi, ni = tables()
    rungs = closed_form_rungs(True, False)
    queue(rec, **{base: UNSUPPORTED for base in rungs[:failing]}, **{rungs[failing]: status})
    with pytest.raises(_lib.HipLibraryError, match=f"^mgp_posterior failed: {text}"):
        fused.posterior_mean_var(spec_of(), Xq, X, bi, ni, Y, packed=True)
    assert names(rec) == rungs[: failing + 1]


def test_closed_form_auto_refused_by_every_rung(rec):
    X, Xq, Y, bi, ni = tables()
    queue(rec, posterior=UNSUPPORTED, posterior_large=UNSUPPORTED)
    with pytest.raises(_lib.HipLibraryError, match="^mgp_posterior failed: MGP_EUNSUPPORTED"):
        fused.posterior_mean_var(spec_of(), Xq, X, bi, ni, Y, packed=False)
    assert names(rec) == ["posterior", "posterior_large"]


def test_closed_form_auto_beyond_1024_rows_is_a_value_error_after_the_plain_call(rec):
    X, Xq, Y, bi, _ = tables()
    ni = torch.randint(0, N, (B, 1022))  # with two responses: 1025 rows
    queue(rec, posterior=UNSUPPORTED)
    with pytest.raises(ValueError, match=rows_message(1022, R)):
        fused.posterior_mean_var(spec_of(), Xq, X, bi, ni, Y, packed=True)  # (k + 1 + R > 64: nothing to pack either)
    assert names(rec) == ["posterior"]


@pytest.mark.parametrize("path, base", [("generic", "posterior_generic"), ("rhs", "posterior_rhs")])
def test_closed_form_named_family_is_that_entry_alone(rec, path, base):
    X, Xq, Y, bi, ni = tables()
    mean, var = fused.posterior_mean_var(spec_of(), Xq, X, bi, ni, Y, path=path, packed=True)
    assert names(rec) == [base] and rec.calls[0][0] == base  # (no table pack: a named family reads the plain tables)
    assert vals(rec.calls[0])[0:9] == [Xq.data_ptr(), X.data_ptr(), D, bi.data_ptr(), ni.data_ptr(), B, K, Y.data_ptr(), R]
    rec.calls.clear()
    queue(rec, **{base: UNSUPPORTED})
    with pytest.raises(_lib.HipLibraryError, match="^mgp_posterior failed: MGP_EUNSUPPORTED"):
        fused.posterior_mean_var(spec_of(), Xq, X, bi, ni, Y, path=path)
    assert names(rec) == [base]  # no slab retry


@pytest.mark.parametrize("gathered", [False, True])
def test_closed_form_path_large_is_the_slab_entry_alone(rec, gathered):
    X, Xq, Y, bi, ni = tables()
    tg = Y[ni] if gathered else Y
    info = torch.zeros(1, dtype=torch.int32)
    mean, var = fused.posterior_mean_var(spec_of(), Xq, X, bi, ni, tg, path="large", packed=True, gathered=gathered, info=info)
    assert [c[0] for c in rec.calls] == ["posterior_large"]
    v = vals(rec.calls[0])
    assert v[0:10] == [Xq.data_ptr(), X.data_ptr(), D, bi.data_ptr(), ni.data_ptr(), B, K, tg.data_ptr(), R, int(gathered)]
    assert v[10:15] == [0, 1e-3, None, 2, 0] and v[15] is not None and v[16] == 3
    assert v[17:21] == [mean.data_ptr(), var.data_ptr(), None, info.data_ptr()]
    check_workspace(rec.calls[0], large_bytes(K, R))
    rec.calls.clear()
    queue(rec, posterior_large=UNSUPPORTED)
    with pytest.raises(_lib.HipLibraryError, match="^mgp_posterior failed: MGP_EUNSUPPORTED"):
        fused.posterior_mean_var(spec_of(), Xq, X, bi, ni, tg, path="large", gathered=gathered)
    assert names(rec) == ["posterior_large"]
    rec.calls.clear()
    with pytest.raises(ValueError, match=rows_message(1022, R)):
        fused.posterior_mean_var(spec_of(), Xq, X, bi, torch.randint(0, N, (B, 1022)), Y, path="large")
    assert rec.calls == []


# ---- posterior_mean_var, general-smoothness Matern --------------------------------------------------------------------

GEN_MESSAGE = r"^general-smoothness Matern: no fused kernel for torch.float32, k={k}, R=2, d=3$"


@pytest.mark.parametrize("packed", [False, True])
def test_general_smoothness_up_to_64_slots_is_one_call(rec, packed):
    """mgp_posterior_gen_*: fq fn packed_q q_stride packed_nn nn_stride d ...: prepared tables when packing applies,
    and no retry on the plain ones."""
    X, Xq, Y, bi, ni = tables()
    queue(rec, posterior_gen=UNSUPPORTED)
    with pytest.raises(FusedUnsupported, match=GEN_MESSAGE.format(k=K)):
        fused.posterior_mean_var(spec_of("matern_gen"), Xq, X, bi, ni, Y, packed=packed)
    assert names(rec) == ["posterior_gen"]
    v = vals(rec.of()[0])
    if packed:
        assert v[0:2] == [None, None] and v[2] is not None and v[4] is not None and v[6] == 4
    else:
        assert v[0:7] == [Xq.data_ptr(), X.data_ptr(), None, 0, None, 0, D]
    rec.calls.clear()
    queue(rec, posterior_gen=EINVAL)
    with pytest.raises(_lib.HipLibraryError, match="^mgp_posterior_gen failed: MGP_EINVAL"):
        fused.posterior_mean_var(spec_of("matern_gen"), Xq, X, bi, ni, Y, packed=packed)
    assert names(rec) == ["posterior_gen"]


@pytest.mark.parametrize("packed", [False, True, "auto"])
def test_general_smoothness_beyond_64_slots_plain_then_slab(rec, packed):
    X, Xq, Y, bi, ni = tables(k=70)
    queue(rec, posterior_gen=UNSUPPORTED)
    mean, var = fused.posterior_mean_var(spec_of("matern_gen"), Xq, X, bi, ni, Y, packed=packed)
    assert [c[0] for c in rec.calls] == ["posterior_gen", "posterior_gen_large"]  # never packed: no table_pack either
    first, second = (vals(c) for c in rec.calls)
    assert first[0:6] == [Xq.data_ptr(), X.data_ptr(), None, 0, None, 0]
    # mgp_posterior_gen_large_*: fq fn d bi ni b k tg R targets_batch noise(3) smoothness metric ls ls_count mean var ykinvy info
    assert second[0:21] == first[0:2] + first[6:25]
    assert second[17:21] == [mean.data_ptr(), var.data_ptr(), None, None]
    check_workspace(rec.calls[1], large_bytes(70, R))
    for status, exc, message in ((UNSUPPORTED, FusedUnsupported, GEN_MESSAGE.format(k=70)),
                                 (EINVAL, _lib.HipLibraryError, "^mgp_posterior_gen failed: MGP_EINVAL")):
        rec.calls.clear()
        queue(rec, posterior_gen=UNSUPPORTED, posterior_gen_large=status)
        with pytest.raises(exc, match=message):
            fused.posterior_mean_var(spec_of("matern_gen"), Xq, X, bi, ni, Y, packed=packed)
        assert [c[0] for c in rec.calls] == ["posterior_gen", "posterior_gen_large"]
    rec.calls.clear()
    queue(rec, posterior_gen=EINVAL)
    with pytest.raises(_lib.HipLibraryError, match="^mgp_posterior_gen failed: MGP_EINVAL"):
        fused.posterior_mean_var(spec_of("matern_gen"), Xq, X, bi, ni, Y, packed=packed)
    assert [c[0] for c in rec.calls] == ["posterior_gen"]


def test_general_smoothness_beyond_1024_rows_makes_no_slab_call(rec):
    X, Xq, Y, bi, _ = tables()
    ni = torch.randint(0, N, (B, 1022))
    queue(rec, posterior_gen=UNSUPPORTED)
    with pytest.raises(FusedUnsupported, match=GEN_MESSAGE.format(k=1022)):
        fused.posterior_mean_var(spec_of("matern_gen"), Xq, X, bi, ni, Y)
    assert [c[0] for c in rec.calls] == ["posterior_gen"]
    rec.calls.clear()
    with pytest.raises(FusedUnsupported, match=GEN_MESSAGE.format(k=1022)):  # by name: not even that call
        fused.posterior_mean_var(spec_of("matern_gen"), Xq, X, bi, ni, Y, path="large")
    assert rec.calls == []


@pytest.mark.parametrize("k", [K, 70])
@pytest.mark.parametrize("path, base", [("generic", "posterior_gen_generic"), ("large", "posterior_gen_large")])
def test_general_smoothness_named_family_is_that_entry_alone(rec, path, base, k):
    X, Xq, Y, bi, ni = tables(k=k)
    mean, var = fused.posterior_mean_var(spec_of("matern_gen"), Xq, X, bi, ni, Y, path=path, packed=True)
    assert [c[0] for c in rec.calls] == [base]
    v = vals(rec.calls[0])
    assert v[0:10] == [Xq.data_ptr(), X.data_ptr(), D, bi.data_ptr(), ni.data_ptr(), B, k, Y.data_ptr(), R, 0]
    assert v[10:15] == [0, 1e-3, None, 0.42, 0] and v[16] == 3 and v[17:21] == [mean.data_ptr(), var.data_ptr(), None, None]
    if path == "large":
        check_workspace(rec.calls[0], large_bytes(k, R))
    else:
        assert len(v) == 22 and v[21] == STREAM
    for status, exc, message in ((UNSUPPORTED, FusedUnsupported, GEN_MESSAGE.format(k=k)),
                                 (EINVAL, _lib.HipLibraryError, "^mgp_posterior_gen failed: MGP_EINVAL")):
        rec.calls.clear()
        queue(rec, **{base: status})
        with pytest.raises(exc, match=message):
            fused.posterior_mean_var(spec_of("matern_gen"), Xq, X, bi, ni, Y, path=path)
        assert [c[0] for c in rec.calls] == [base]


# ---- loocv_partials ---------------------------------------------------------------------------------------------------

def loocv(rec, packed, kernel="matern15", k=K):
    X, _, y, _, ni = tables(k=k, one_response=True)
    bi = torch.arange(B)
    info = torch.zeros(1, dtype=torch.int32)
    run = lambda: fused.loocv_partials(spec_of(kernel), X, y, bi, ni, huber_delta=1.25, packed=packed, info=info,  # noqa: E731
                                       return_ykinvy=True)
    return X, y, bi, ni, info, run


@pytest.mark.parametrize("packed", [False, True])
def test_loocv_prepared_plain_slab_then_the_tree(rec, resets, packed):
    X, y, bi, ni, info, run = loocv(rec, packed)
    rungs = (["loocv_packed"] if packed else []) + ["loocv", "posterior_large", "loocv_tree"]
    queue(rec, loocv_packed=UNSUPPORTED, loocv=UNSUPPORTED)
    partials, mean, var, yk = run()
    assert names(rec) == rungs and resets == []
    plain, large, tree = (vals(c) for c in rec.of()[-3:])
    # mgp_loocv_*: feat d bi ni b k tg | noise(3) kernel metric ls ls_count | mean var ykinvy info | huber partials scratch stream
    assert plain[0:7] == [X.data_ptr(), D, bi.data_ptr(), ni.data_ptr(), B, K, y.data_ptr()]
    assert large[0:10] == [plain[0], plain[0]] + plain[1:7] + [1, 0]     # both sides the training table, the (n, 1) table
    assert large[10:21] == plain[7:18] == [0, 1e-3, None, 2, 0, plain[12], 3, mean.data_ptr(), var.data_ptr(), yk.data_ptr(),
                                           info.data_ptr()]
    check_workspace(rec.of()[-2], large_bytes(K, 1))
    # mgp_loocv_tree_*: mean var ykinvy resp resp_stride_bytes bi b huber grid nh partials scratch stream
    assert tree[0:10] == [mean.data_ptr(), var.data_ptr(), yk.data_ptr(), y.data_ptr(), 4, bi.data_ptr(), B, 1.25, 0, 0]
    assert tree[10] == partials.data_ptr() != plain[19] and tree[11] is not None and tree[12] == STREAM
    assert partials.shape == (6,) and partials.dtype == torch.float64
    if packed:
        first = vals(rec.of()[0])
        assert first[3:7] == plain[2:6] and first[7:12] == plain[7:12] and first[14:] == plain[14:]


@pytest.mark.parametrize("status, text", [(UNSUPPORTED, "MGP_EUNSUPPORTED"), (EINVAL, "MGP_EINVAL")])
def test_loocv_a_failing_slab_rung_is_named_mgp_posterior_large(rec, resets, status, text):
    *_, run = loocv(rec, False)
    queue(rec, loocv=UNSUPPORTED, posterior_large=status)
    with pytest.raises(_lib.HipLibraryError, match=f"^mgp_posterior_large failed: {text}"):
        run()
    assert names(rec) == ["loocv", "posterior_large"] and resets == []


def test_loocv_a_failing_tree_is_named_mgp_loocv_tree(rec, resets):
    *_, run = loocv(rec, False)
    queue(rec, loocv=UNSUPPORTED, loocv_tree=EINVAL)
    with pytest.raises(_lib.HipLibraryError, match="^mgp_loocv_tree failed: MGP_EINVAL"):
        run()
    assert names(rec) == ["loocv", "posterior_large", "loocv_tree"] and resets == []


@pytest.mark.parametrize("failing", ["loocv_packed", "loocv"])
def test_loocv_any_other_status_resets_the_scratch_and_is_named_mgp_loocv(rec, resets, failing):
    *_, run = loocv(rec, True)
    queue(rec, loocv_packed=UNSUPPORTED)
    queue(rec, **{failing: EINVAL})
    with pytest.raises(_lib.HipLibraryError, match="^mgp_loocv failed: MGP_EINVAL"):
        run()
    assert names(rec) == ["loocv_packed", "loocv"][: 1 + (failing == "loocv")] and resets == [1]


def test_loocv_general_smoothness_has_no_slab_rung(rec, resets):
    *_, run = loocv(rec, True, kernel="matern_gen")
    queue(rec, loocv_packed=UNSUPPORTED, loocv=UNSUPPORTED)
    with pytest.raises(_lib.HipLibraryError, match="^mgp_loocv failed: MGP_EUNSUPPORTED"):
        run()
    assert names(rec) == ["loocv_packed", "loocv"] and resets == [1]


def test_loocv_beyond_1024_rows_is_a_value_error_after_the_plain_call(rec, resets):
    *_, run = loocv(rec, True, k=1023)
    queue(rec, loocv=UNSUPPORTED)
    with pytest.raises(ValueError, match=rows_message(1023, 1)):
        run()
    assert names(rec) == ["loocv"] and resets == []


# ---- _hyper_partials --------------------------------------------------------------------------------------------------

def backward_bytes(k):
    return _lib.load().mgp_backward_large_workspace_bytes(4, k, B)


def loocv_gradient(k=K):
    X, _, y, _, ni = tables(k=k, one_response=True)
    # (a loss and a scale that divide by none of the sums: the recorder leaves the forward's outputs unwritten)
    return lambda: fused.loocv_value_and_grad(spec_of(), X, y, torch.arange(B), ni, loss="pseudo_huber", packed=False,
                                              scale=("fixed", 1.0))


def class_gradient(k=K):
    X, _, Y, _, ni = tables(k=k)
    return lambda: fused.class_value_and_grad(spec_of(), X, Y, torch.arange(B), ni, packed=False)


SUMS = ("column_sums", "class_sums")


def test_hyper_partials_of_the_loocv_objective(rec):
    queue(rec, loocv_backward=UNSUPPORTED)
    value, g_l, g_n = loocv_gradient()()
    assert names(rec, *SUMS) == ["loocv", "loocv_backward", "hyper_backward_large"] and g_l.shape == (3,)
    first, second = (vals(c) for c in rec.of(*SUMS)[1:])
    # mgp_loocv_backward_*: feat d bi ni b k tg | noise(3) kernel metric ls ls_count | gm gv gyk | g_ls g_noise info | stream
    # mgp_hyper_backward_large_*: ... tg R | the same | workspace workspace_bytes stream
    assert len(first) == 21 and second[0:7] == first[0:7] and second[7] == 1 and second[8:21] == first[7:20]
    assert first[7:11] == [0, 1e-3, None, 2] and None not in first[14:19] and first[20] == STREAM
    check_workspace(rec.of(*SUMS)[2], backward_bytes(K))


def test_hyper_partials_of_the_classification_objective(rec):
    queue(rec, posterior_backward=UNSUPPORTED)
    value, g_l, g_n = class_gradient()()
    assert names(rec, *SUMS) == ["posterior", "posterior_backward", "hyper_backward_large"]
    first, second = (vals(c) for c in rec.of(*SUMS)[1:])
    # mgp_posterior_backward_*: fq fn d bi ni b k tg R | noise(3) kernel metric ls ls_count | gm gv | g_q g_x g_t | g_ls g_noise
    # info | stream
    assert len(first) == 25 and first[0] == first[1] and second[0:8] == first[1:9] and second[7] == R
    assert second[8:15] == first[9:16] and second[15:17] == first[16:18] and second[17] is None
    assert first[17] is None and first[18:21] == [None, None, None] and second[18:21] == first[21:24]
    check_workspace(rec.of(*SUMS)[2], backward_bytes(K))


@pytest.mark.parametrize("gradient, first", [(loocv_gradient, "loocv_backward"), (class_gradient, "posterior_backward")])
def test_hyper_partials_error_is_named_after_the_rung_that_failed(rec, gradient, first):
    queue(rec, **{first: EINVAL})
    with pytest.raises(_lib.HipLibraryError, match=f"^mgp_{first} failed: MGP_EINVAL"):
        gradient()()
    assert names(rec, *SUMS)[1:] == [first]
    for status, text in ((EINVAL, "MGP_EINVAL"), (UNSUPPORTED, "MGP_EUNSUPPORTED")):
        rec.calls.clear()
        queue(rec, **{first: UNSUPPORTED}, hyper_backward_large=status)
        with pytest.raises(_lib.HipLibraryError, match=f"^mgp_hyper_backward_large failed: {text}"):
            gradient()()
        assert names(rec, *SUMS)[1:] == [first, "hyper_backward_large"]


def test_hyper_partials_beyond_1024_rows_is_a_value_error_after_the_lds_call(rec):
    queue(rec, loocv_backward=UNSUPPORTED)
    message = (rf"nn_count = 1023 exceeds the limit of the analytic hyper-parameter gradient, mgp_large_max_nn_count = "
               rf"{_lib.load().mgp_large_max_nn_count(4, 1)} \(a local system holds at most 1024 rows: nn_count \+ 2 in the backward\)")
    with pytest.raises(ValueError, match=message):
        loocv_gradient(k=1023)()
    assert names(rec, *SUMS)[1:] == ["loocv_backward"]


# ---- autograd._FusedPosterior.forward ---------------------------------------------------------------------------------

def autograd_forward(k=K):
    X, Xq, Y, bi, ni = tables(k=k)
    ls, noise = torch.tensor([2.0, 3.0, 4.0]), torch.tensor(1e-3)
    run = lambda: autograd._FusedPosterior.apply(Xq, X, Y, ls, noise, bi, ni, 2, 0, False, False)  # noqa: E731
    return X, Xq, Y, bi, ni, ls, noise, run


def test_autograd_forward_lds_then_slab(rec):
    X, Xq, Y, bi, ni, ls, noise, run = autograd_forward()
    queue(rec, posterior=UNSUPPORTED)
    mean, var = run()
    assert names(rec) == ["posterior", "posterior_large"]
    plain, large = rec.calls
    p = vals(plain)
    assert p[0:9] == [Xq.data_ptr(), X.data_ptr(), D, bi.data_ptr(), ni.data_ptr(), B, K, Y.data_ptr(), R]
    # the noise tensor decoded inside the function; ykinvy NULL, an info counter of the function's own
    assert p[9:16] == [0, float(noise), None, 2, 0, ls.data_ptr(), 3]
    assert p[16:19] == [mean.data_ptr(), var.data_ptr(), None] and p[19] is not None and p[20] == STREAM
    check_plain_then_large(plain, large, gathered=False)
    check_workspace(large, large_bytes(K, R))


def test_autograd_forward_error_is_named_after_the_rung_that_failed(rec):
    *_, run = autograd_forward()
    queue(rec, posterior=EINVAL)
    with pytest.raises(_lib.HipLibraryError, match="^mgp_posterior failed: MGP_EINVAL"):
        run()
    assert names(rec) == ["posterior"]
    for status, text in ((EINVAL, "MGP_EINVAL"), (UNSUPPORTED, "MGP_EUNSUPPORTED")):
        rec.calls.clear()
        queue(rec, posterior=UNSUPPORTED, posterior_large=status)
        with pytest.raises(_lib.HipLibraryError, match=f"^mgp_posterior_large failed: {text}"):
            run()
        assert names(rec) == ["posterior", "posterior_large"]
    rec.calls.clear()
    *_, run = autograd_forward(k=1022)
    queue(rec, posterior=UNSUPPORTED)
    with pytest.raises(ValueError, match=rows_message(1022, R)):
        run()
    assert names(rec) == ["posterior"]


# ---- _solve on materialised systems -----------------------------------------------------------------------------------

def test_solve_lds_then_slab_named_mgp_solve_either_way(rec):
    g = torch.Generator().manual_seed(3)
    Kin, Kcross, Y = torch.randn(B, K, K, generator=g), torch.randn(B, K, generator=g), torch.randn(B, K, R, generator=g)
    want = ("mean", "var", "ykinvy", "coeffs")
    queue(rec, solve=UNSUPPORTED)
    mean, var, yk, co = M._solve(Kin, Kcross, Y, kout=1.5, want=want)
    assert names(rec) == ["solve", "solve_large"]
    first, second = (vals(c) for c in rec.calls)
    # mgp_solve_*: Kin Kcross Y b k R kout mean var ykinvy coeffs info stream
    assert first[0:11] == [Kin.data_ptr(), Kcross.data_ptr(), Y.data_ptr(), B, K, R, 1.5, mean.data_ptr(), var.data_ptr(),
                           yk.data_ptr(), co.data_ptr()]
    assert len(first) == 13 and first[11] is not None and first[12] == STREAM and second[0:12] == first[0:12]
    check_workspace(rec.calls[1], large_bytes(K, R))
    for statuses, rungs in ((dict(solve=EINVAL), ["solve"]), (dict(solve=UNSUPPORTED, solve_large=EINVAL), ["solve", "solve_large"])):
        rec.calls.clear()
        queue(rec, **statuses)
        with pytest.raises(_lib.HipLibraryError, match="^mgp_solve failed: MGP_EINVAL"):
            M._solve(Kin, Kcross, Y, want=want)
        assert names(rec) == rungs
    rec.calls.clear()
    queue(rec, solve=UNSUPPORTED, solve_large=UNSUPPORTED)
    with pytest.raises(_lib.HipLibraryError, match="^mgp_solve failed: MGP_EUNSUPPORTED"):
        M._solve(Kin, Kcross, Y, want=want)
    rec.calls.clear()
    queue(rec, solve=UNSUPPORTED)
    with pytest.raises(ValueError, match=rows_message(1023, 1)):
        M._solve(torch.zeros(2, 1023, 1023), None, torch.zeros(2, 1023, 1), want=("coeffs",))
    assert names(rec) == ["solve"]
