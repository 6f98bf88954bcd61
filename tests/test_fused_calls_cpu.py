"""CPU: what the fused Python functions hand the C entry points, argument by argument.

``muygpys_amd._lib.fn`` is replaced by a recorder, so every call stops at the library boundary: the entry point's
name and its argument list are compared with the parameter order of include/muygpys_hip.h, written out here
position by position.  CPU tensors have a ``data_ptr()``, so the marshalling itself runs for real; only the device
check, the stream and the LOOCV scratch are stood in for.  ``mgp_packed_row_bytes`` (a host function) is the library's.

Shapes: fp32, k = 5, d = 3, R = 2, b = 7 -- a prepared table pads the 12-byte feature rows to d_kernel = 4, so the
prepared-table calls carry d = 4, a 64-byte stride and (Anisotropy) four length scales."""

import pytest
import torch

from muygpys_amd import _lib, fused
from muygpys_amd.fused import FusedUnsupported, KernelSpec
from tests.call_recorder import STREAM, install, vals

K, D, R, B, N, NQ = 5, 3, 2, 7, 40, 9
STRIDE = 64  # mgp_packed_row_bytes(4, R <= 4, 4): 16 bytes of features + the 16-byte response slot, to 64
F32 = torch.float32


@pytest.fixture
def rec(monkeypatch):
    yield install(monkeypatch)
    fused.clear_caches()


def tables(n=N, nq=NQ, b=B, one_response=False, seed=0):
    g = torch.Generator().manual_seed(seed)
    X = torch.randn(n, D, generator=g)
    Xq = torch.randn(nq, D, generator=g)
    Y = torch.randn(n, generator=g) if one_response else torch.randn(n, R, generator=g)
    bi = torch.randint(0, nq, (b,), generator=g)
    ni = torch.randint(0, n, (b, K), generator=g)
    return X, Xq, Y, bi, ni


def spec_of(kernel, ls=(2.0, 3.0, 4.0), noise=1e-3):
    return KernelSpec(kernel, "l2", ls, noise, smoothness=0.42 if kernel == "matern_gen" else None)


# ---- posterior_mean_var -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kernel", ["matern15", "matern_gen"])
@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("gathered", [False, True])
def test_posterior_call_by_table_form(rec, gathered, packed, kernel):
    X, Xq, Y, bi, ni = tables()
    tg = Y[ni] if gathered else Y
    mean_buf, var_buf = torch.empty(B, R), torch.empty(B)
    mean, var, yk = fused.posterior_mean_var(spec_of(kernel), Xq, X, bi, ni, tg, want_ykinvy=True, out_mean=mean_buf,
                                             out_var=var_buf, packed=packed, gathered=gathered)
    assert mean.shape == (B, R) and var.shape == (B,) and yk.shape == (B, R)
    assert mean.data_ptr() == mean_buf.data_ptr() and var.data_ptr() == var_buf.data_ptr()
    calls = rec.of()
    assert len(calls) == 1 and calls[0][1] == F32
    base, v = calls[0][0], vals(calls[0])
    if packed:
        pn = fused.pack_table(X, None if gathered else Y, query=False)  # (cache hits: the tables the call made)
        pq = fused.pack_table(Xq, None)
        assert (pn.stride, pq.stride, pn.d_kernel) == (STRIDE, STRIDE, 4) and pn.data.data_ptr() != pq.data.data_ptr()
        tabs = [pq.data.data_ptr(), STRIDE, pn.data.data_ptr(), STRIDE]
    d, lsc = (4, 4) if packed else (3, 3)
    ls_at = None
    if kernel == "matern_gen":
        # fq, fn, packed_q, q_stride, packed_nn, nn_stride, d, bi, ni, b, k, tg, R, targets_batch, noise_mode, eps, nd,
        # smoothness, metric, ls, ls_count, mean, var, ykinvy, info, stream
        assert base == "posterior_gen" and len(v) == 26
        assert v[0:2] == ([None, None] if packed else [Xq.data_ptr(), X.data_ptr()])
        assert v[2:6] == (tabs if packed else [None, 0, None, 0])
        # (`tg` is passed also where the prepared table carries the responses)
        assert v[6:17] == [d, bi.data_ptr(), ni.data_ptr(), B, K, tg.data_ptr(), R, int(gathered), 0, 1e-3, None]
        assert v[17:19] == [0.42, 0]
        ls_at, out_at = 19, 21
    elif not packed:
        # fq, fn, d, bi, ni, b, k, tg, R, noise_mode, eps, nd, kernel, metric, ls, ls_count, mean, var, ykinvy, info, stream
        assert base == ("posterior_gathered" if gathered else "posterior") and len(v) == 21
        assert v[0:14] == [Xq.data_ptr(), X.data_ptr(), 3, bi.data_ptr(), ni.data_ptr(), B, K, tg.data_ptr(), R, 0, 1e-3,
                           None, 2, 0]
        ls_at, out_at = 14, 16
    elif gathered:
        # packed_q, q_stride, packed_nn, nn_stride, d, bi, ni, b, k, nn_tg, R, noise_mode, eps, nd, kernel, metric, ls, ...
        assert base == "posterior_packed_gathered" and len(v) == 23
        assert v[0:16] == tabs + [4, bi.data_ptr(), ni.data_ptr(), B, K, tg.data_ptr(), R, 0, 1e-3, None, 2, 0]
        ls_at, out_at = 16, 18
    else:
        # packed_q, q_stride, packed_nn, nn_stride, d, bi, ni, b, k, R, noise_mode, eps, nd, kernel, metric, ls, ...
        assert base == "posterior_packed" and len(v) == 22
        assert v[0:15] == tabs + [4, bi.data_ptr(), ni.data_ptr(), B, K, R, 0, 1e-3, None, 2, 0]
        ls_at, out_at = 15, 17
    assert v[ls_at] is not None and v[ls_at + 1] == lsc
    assert v[out_at:] == [mean_buf.data_ptr(), var_buf.data_ptr(), yk.data_ptr(), None, STREAM]


@pytest.mark.parametrize("path, base", [("generic", "posterior_generic"), ("rhs", "posterior_rhs")])
def test_posterior_call_on_a_named_kernel_family(rec, path, base):
    X, Xq, Y, bi, ni = tables(one_response=True)
    info = torch.zeros(1, dtype=torch.int32)
    mean, var = fused.posterior_mean_var(spec_of("matern15", ls=2.0), Xq, X, bi, ni, Y, path=path, packed=False, info=info)
    assert mean.shape == (B,) and var.shape == (B,)  # 1-D targets: no response axis
    (call,) = rec.of()
    v = vals(call)
    assert call[0] == base
    assert v[0:14] == [Xq.data_ptr(), X.data_ptr(), 3, bi.data_ptr(), ni.data_ptr(), B, K, Y.data_ptr(), 1, 0, 1e-3, None, 2, 0]
    assert v[14] is not None and v[15] == 1                      # Isotropy: one length scale
    assert v[16] == mean.data_ptr() and v[17] == var.data_ptr()
    assert v[18:] == [None, info.data_ptr(), STREAM]             # no ykinvy asked for


def test_posterior_noise_modes_and_squeeze_of_gathered_responses(rec):
    X, Xq, Y, bi, ni = tables(one_response=True)
    table, batch = torch.rand(N), torch.rand(B, K)
    for noise, mode in ((table, 1), (batch, 2)):
        rec.calls.clear()
        mean, var, yk = fused.posterior_mean_var(spec_of("matern15", noise=noise), Xq, X, None, ni, Y[ni], packed=False,
                                                 gathered=True, want_ykinvy=True)
        assert mean.shape == (B,) and yk.shape == (B,)  # (b, k) gathered responses: no response axis
        (call,) = rec.of()
        v = vals(call)
        assert call[0] == "posterior_gathered" and v[3] is None  # batch_indices None -> NULL
        assert v[8:12] == [1, mode, 0.0, noise.data_ptr()]


@pytest.mark.parametrize("gathered", [False, True])
def test_unsupported_prepared_tables_retry_the_plain_tables(rec, gathered):
    X, Xq, Y, bi, ni = tables()
    packed_base, plain_base = ("posterior_packed_gathered", "posterior_gathered") if gathered else ("posterior_packed", "posterior")
    rec.statuses[packed_base] = [-2]
    tg = Y[ni] if gathered else Y
    fused.posterior_mean_var(spec_of("matern15"), Xq, X, bi, ni, tg, packed=True, gathered=gathered)
    first, second = rec.of()
    assert first[0] == packed_base and vals(first)[4] == 4
    v = vals(second)
    assert second[0] == plain_base
    assert v[0:9] == [Xq.data_ptr(), X.data_ptr(), 3, bi.data_ptr(), ni.data_ptr(), B, K, tg.data_ptr(), R]  # d = 3, not 4
    assert v[15] == 3                                                                                        # ... and 3 scales


@pytest.mark.parametrize("packed", [False, True])
def test_unsupported_general_smoothness_raises_without_a_retry(rec, packed):
    X, Xq, Y, bi, ni = tables()
    rec.statuses["posterior_gen"] = [-2]
    with pytest.raises(FusedUnsupported, match="general-smoothness Matern: no fused kernel"):
        fused.posterior_mean_var(spec_of("matern_gen"), Xq, X, bi, ni, Y, packed=packed)
    assert [c[0] for c in rec.of()] == ["posterior_gen"]  # prepared tables: NOT tried again on the plain ones


def test_a_failed_call_raises_the_library_error(rec):
    X, Xq, Y, bi, ni = tables()
    rec.statuses["posterior"] = [-1]
    with pytest.raises(_lib.HipLibraryError, match="mgp_posterior failed: MGP_EINVAL"):
        fused.posterior_mean_var(spec_of("matern15"), Xq, X, bi, ni, Y, packed=False)


def test_auto_packs_from_a_quarter_of_the_rows_or_on_a_cache_hit(rec):
    """packed="auto": b (k + 1) = 42 gathered rows against rows // 4 of the tables a pack would pass over."""
    def served(n, nq=None, prepare=False):
        fused.clear_caches()
        rec.calls.clear()
        X, Xq, Y, bi, ni = tables(n=n, nq=nq or NQ)
        if prepare:
            fused.pack_table(X, Y)
        bi = torch.arange(B)
        fused.posterior_mean_var(spec_of("matern15"), X if nq is None else Xq, X, bi, ni, Y)
        (call,) = rec.of()
        return call[0]

    assert served(171) == "posterior_packed"       # 171 // 4 = 42: exactly at the threshold
    assert served(172) == "posterior"              # 172 // 4 = 43: one below it
    assert served(172, prepare=True) == "posterior_packed"   # the table is there already
    assert served(160, nq=11) == "posterior_packed"          # a separate test table counts: (160 + 11) // 4 = 42
    assert served(160, nq=12) == "posterior"                 # (160 + 12) // 4 = 43


# ---- LOOCV ------------------------------------------------------------------------------------------------------------

# mgp_loocv_*:        feat, d, bi, ni, b, k, tg, noise_mode, eps, nd, kernel, metric, ls, ls_count, mean, var, ykinvy, info,
#                     huber_delta, partials, scratch, stream
# mgp_loocv_packed_*: packed, stride, d, bi, ni, b, k, noise_mode, ... (the same from there on)

def loocv_case(rec, packed, ls=2.0):
    X, _, y, _, ni = tables(one_response=True)
    bi = torch.arange(B)
    info = torch.zeros(1, dtype=torch.int32)
    out = fused.loocv_partials(spec_of("matern15", ls=ls), X, y, bi, ni, huber_delta=1.25, packed=packed, info=info,
                               return_ykinvy=True)
    return X, y, bi, ni, info, out


@pytest.mark.parametrize("packed", [False, True])
def test_loocv_partials_call(rec, packed):
    X, y, bi, ni, info, (partials, mean, var, yk) = loocv_case(rec, packed, ls=(2.0, 3.0, 4.0))
    assert partials.shape == (6,) and partials.dtype == torch.float64 and mean.shape == var.shape == yk.shape == (B,)
    (call,) = rec.of()
    v = vals(call)
    assert len(v) == 22
    if packed:
        pn = fused.pack_table(X, y)
        assert call[0] == "loocv_packed" and v[0:7] == [pn.data.data_ptr(), STRIDE, 4, bi.data_ptr(), ni.data_ptr(), B, K]
    else:
        assert call[0] == "loocv" and v[0:7] == [X.data_ptr(), 3, bi.data_ptr(), ni.data_ptr(), B, K, y.data_ptr()]
    assert v[7:12] == [0, 1e-3, None, 2, 0]
    assert v[12] is not None and v[13] == (4 if packed else 3)
    assert v[14:20] == [mean.data_ptr(), var.data_ptr(), yk.data_ptr(), info.data_ptr(), 1.25, partials.data_ptr()]
    assert v[20] is not None and v[21] == STREAM


def test_loocv_partials_retries_the_plain_table(rec):
    rec.statuses["loocv_packed"] = [-2]
    X, y, bi, ni, info, _ = loocv_case(rec, True, ls=(2.0, 3.0, 4.0))
    first, second = rec.of()
    assert first[0] == "loocv_packed" and second[0] == "loocv"
    v = vals(second)
    assert v[0:7] == [X.data_ptr(), 3, bi.data_ptr(), ni.data_ptr(), B, K, y.data_ptr()] and v[13] == 3
    assert vals(first)[7:12] == v[7:12] and vals(first)[14:] == v[14:]


@pytest.mark.parametrize("packed", [False, True])
def test_loocv_plan_prepares_the_call_loocv_partials_makes(rec, packed):
    """Position by position, apart from the buffers a plan owns: its length-scale word, outputs, info, sums, scratch."""
    X, y, bi, ni, info, _ = loocv_case(rec, packed)
    (direct,) = rec.of()
    rec.calls.clear()
    plan = fused.LoocvPlan("matern15", "l2", X, y, bi, ni, huber_delta=1.25, packed=packed)
    assert rec.of() == []  # nothing is launched by the preparation
    plan.launch(2.0, 1e-3)
    (planned,) = rec.of()
    assert planned[0] == direct[0] == ("loocv_packed" if packed else "loocv")
    want, got = vals(direct), vals(planned)
    own = {12, 14, 15, 16, 17, 19, 20}
    assert len(got) == len(want) == 22
    for i in range(22):
        if i in own:
            assert got[i] is not None, i
        else:
            assert got[i] == want[i], (i, got[i], want[i])
    assert got[13] == 1 and got[8] == 1e-3
    assert got[14:18] == [plan.mean.data_ptr(), plan.var.data_ptr(), plan.ykinvy.data_ptr(), plan.info.data_ptr()]
    assert got[19] == plan.partials.data_ptr() and got[20] == plan.scratch.data_ptr()
    # "auto" has no row threshold in a plan: it packs where the shape allows, however small the batch
    small = fused.LoocvPlan("matern15", "l2", torch.randn(4000, D), torch.randn(4000), bi, ni)
    rec.calls.clear()
    small.launch(2.0)
    assert rec.of()[0][0] == "loocv_packed"


# ---- the fast posterior mean ------------------------------------------------------------------------------------------

def test_fast_posterior_mean_call(rec):
    # fq, fn, d, bi, ni, b, k, coeffs, coeff_rows, R, kernel, metric, ls, ls_count, mean, stream
    X, Xq, _, bi, ni = tables()
    coeffs, crow = torch.randn(N, K, R), torch.randint(0, N, (B,))
    mean = fused.fast_posterior_mean(spec_of("matern15"), Xq, X, bi, ni, coeffs, crow)
    assert mean.shape == (B, R)
    (call,) = rec.of()
    v = vals(call)
    assert call[0] == "fast_posterior_mean" and len(v) == 16
    assert v[0:12] == [Xq.data_ptr(), X.data_ptr(), 3, bi.data_ptr(), ni.data_ptr(), B, K, coeffs.data_ptr(), crow.data_ptr(),
                       R, 2, 0]
    assert v[12] is not None and v[13:] == [3, mean.data_ptr(), STREAM]
    rec.calls.clear()
    assert fused.fast_posterior_mean(spec_of("matern15"), Xq, X, None, ni, coeffs[:, :, 0].contiguous(), crow).shape == (B,)
    assert vals(rec.of()[0])[3] is None and vals(rec.of()[0])[9] == 1
    rec.statuses["fast_posterior_mean"] = [-2]
    with pytest.raises(FusedUnsupported):
        fused.fast_posterior_mean(spec_of("matern15"), Xq, X, bi, ni, coeffs, crow)


def test_fast_coefficients_fused_call(rec):
    # fn, d, ni, b, k, tg, noise_mode, eps, nd, kernel, metric, ls, ls_count, coeffs, info, stream
    X, _, y, _, _ = tables(one_response=True)
    nn = torch.randint(0, N, (N, K))
    out, nn_fast = fused.fast_coefficients(spec_of("matern15"), X, y, nn)
    assert out.shape == (N, K) and nn_fast.shape == (N, K)
    assert torch.equal(nn_fast[:, 0], torch.arange(N)) and torch.equal(nn_fast[:, 1:], nn[:, :-1])
    (call,) = rec.of()
    v = vals(call)
    assert call[0] == "fast_coefficients" and len(v) == 16
    assert v[0:11] == [X.data_ptr(), 3, nn_fast.data_ptr(), N, K, y.data_ptr(), 0, 1e-3, None, 2, 0]
    assert v[11] is not None and v[12] == 3 and v[13] == out.data_ptr() and v[14] is not None and v[15] == STREAM


# ---- what the functions refuse before any call ------------------------------------------------------------------------

def test_validation_failures(rec):
    X, Xq, Y, bi, ni = tables()
    y = Y[:, 0].contiguous()
    s = spec_of("matern15")
    pmv, lp = fused.posterior_mean_var, fused.loocv_partials
    rows = torch.arange(B)
    cases = [
        (TypeError, "features and targets must share one float dtype", lambda: pmv(s, Xq, X, bi, ni, Y.double())),
        (TypeError, "features and targets must share one float dtype", lambda: pmv(s, Xq.double(), X, bi, ni, Y)),
        (TypeError, "features and targets must share one float dtype", lambda: lp(s, X, y.double(), rows, ni)),
        (ValueError, "test and train features differ in feature count", lambda: pmv(s, Xq[:, :2], X, bi, ni, Y)),
        (ValueError, "train_features and train_targets differ in row count", lambda: pmv(s, Xq, X, bi, ni, Y[:-1])),
        (ValueError, "train_features and train_targets differ in row count", lambda: lp(s, X, y[:-1], rows, ni)),
        (ValueError, r"batch_indices must have shape \(batch_count,\)", lambda: pmv(s, Xq, X, bi[:-1], ni, Y)),
        (ValueError, r"batch_indices must have shape \(batch_count,\)", lambda: lp(s, X, y, rows[:-1], ni)),
        (ValueError, r"7 neighbourhoods but only 6 query rows \(batch_indices is None\)", lambda: pmv(s, Xq[:6], X, None, ni, Y)),
        (ValueError, r"gathered responses must have shape \(7, 5\[, R\]\), got \(7, 4, 2\)",
         lambda: pmv(s, Xq, X, bi, ni, Y[ni][:, :4], gathered=True)),
        (NotImplementedError, "the LOOCV losses are defined for a single response", lambda: lp(s, X, Y, rows, ni)),
        (NotImplementedError, "the LOOCV losses are defined for a single response",
         lambda: fused.LoocvPlan("matern15", "l2", X, Y, rows, ni)),
        (NotImplementedError, "the LOOCV losses are defined for a single response",
         lambda: fused.loocv_value_and_grad(s, X, Y, rows, ni)),
        (NotImplementedError, "the classification losses are defined for two or more response columns",
         lambda: fused.class_value_and_grad(s, X, Y[:, :1], rows, ni)),
        (NotImplementedError, "the classification losses are defined for two or more response columns",
         lambda: fused.class_value_and_grad(s, X, y, rows, ni)),
        (ValueError, "per-training-point noise table holds 39 entries for 40 training points",
         lambda: pmv(spec_of("matern15", noise=torch.rand(N - 1)), Xq, X, bi, ni, Y)),
        (ValueError, r"heteroscedastic noise tensor must have shape \(7, 5\), got \(7, 4\)",
         lambda: pmv(spec_of("matern15", noise=torch.rand(B, K - 1)), Xq, X, bi, ni, Y)),
        (ValueError, r"heteroscedastic noise tensor must have shape \(7, 5\), got \(7, 4\)",
         lambda: lp(spec_of("matern15", noise=torch.rand(B, K - 1)), X, y, rows, ni)),
        (ValueError, r"Difference tensor of shape \(\.\.\., 3\) must have final dimension size of 2",
         lambda: pmv(spec_of("matern15", ls=(1.0, 2.0)), Xq, X, bi, ni, Y)),
        (ValueError, r"Difference tensor of shape \(\.\.\., 3\) must have final dimension size of 2",
         lambda: lp(spec_of("matern15", ls=torch.tensor([1.0, 2.0])), X, y, rows, ni)),
        (ValueError, "unknown kernel path 'wide'", lambda: pmv(s, Xq, X, bi, ni, Y, path="wide")),
        (ValueError, r"the general-smoothness Matern goes through the dispatcher \(path='auto'\)",
         lambda: pmv(spec_of("matern_gen"), Xq, X, bi, ni, Y, path="rhs")),
        (ValueError, "kernel 'matern_gen' needs a positive smoothness, got None",
         lambda: pmv(KernelSpec("matern_gen", "l2", 2.0, 1e-3), Xq, X, bi, ni, Y)),
        (ValueError, r"gathered responses go through the dispatcher \(path='auto'\)",
         lambda: pmv(s, Xq, X, bi, ni, Y[ni], path="rhs", gathered=True)),
    ]
    for exc, message, call in cases:
        with pytest.raises(exc, match=message):
            call()
    assert rec.of() == []  # all of it before the library is called
