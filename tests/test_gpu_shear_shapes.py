"""The packed-lower-triangle kernel family of mgp_shear.hip (shear_tensor_kernel, solve_multi_kernel and the fused
shear_posterior_kernel) at the shapes where such kernels go wrong, against the fp64 numpy oracle on the
well-conditioned problems of tests/shear_cases.py (conditions asserted in tests/test_shear_cases_cpu.py):

  * partial last elimination blocks (n % 4 = 1, 2, 3 and n < 4) on the packed rows, for both models;
  * both sides of the 64 / 256-thread switch and of a 64 KiB LDS request, and the capacity limit itself;
  * workgroups that take a second neighbourhood (b above the persistent grid), with true nearest neighbours, so that
    a block left over or misplaced changes the answer;
  * every output (ykinvy included), every argument form of the C ABI (table / gathered / strided responses,
    batch_idx == NULL, NULL outputs), both noise modes of the 3-in model, solve_multi at m != 3, R = 0 and R > 1.

Tolerances, project metric |a - b| <= t |b| + t rms(b):

  fp64  t = 1e-9 on the shear problems (cond <= 1e3, n <= 274: n cond u is about 3e-11 for the kernel and for the
        oracle's LU alike), 1e-12 for shear_tensor and for solve_multi on its cond ~ 16 systems.  ``Kout - kk`` is held
        to the absolute error allowed to kk, not to its own (cancelled) size.
  fp32  each case is calibrated: e_cal is the error, in the same metric, of a plain numpy fp32 implementation of the
        same operation (shear_cases.posterior_in_dtype / tensor_in_dtype / solve_in_dtype at float32) against the
        fp64 oracle, and the kernel must stay within F max(e_cal, 4 * 2^-23) and never above the project's 1e-3.
        F is the next power of two at or above twice the worst ratio measured on the MI355X:

            fused posterior  mean 1.33 (3-in, homoscedastic, k = 5), kk 1.27 (3-in, k = 21), ykinvy 1.35 (3-in,
                             k = 91); through MuyGPS 1.14; healthy rows of the singular test 1.06     F = 4
            solve_multi      mean 1.59 (n = 13, m = 3, R = 16), kk 1.37 and ykinvy 1.19 (n = 5)            F = 4
            shear_tensor     1.07 (kin23, (2, 33, 33))                                                     F = 4

        The ratios sit near 1 because on these inputs most of an fp32 result's error is the rounding of the inputs
        to fp32, which the kernel and the plain implementation share.  The worst fp64 errors measured were 1.6e-13
        (fused posterior), 2.8e-15 (solve_multi) and 1.6e-15 (shear_tensor).

Forms of one fused-posterior case: all four use the same queries and responses, so mean, kk and ykinvy are asserted
bit-equal across all of them."""

import numpy as np
import pytest

from tests import shear_cases as S
from tests import shear_oracle as O

torch = pytest.importorskip("torch")
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a ROCm device")]

DEV = "cuda"
DTYPES = ["float64", "float32"]
F_POSTERIOR, F_SOLVE, F_TENSOR = 4.0, 4.0, 4.0
UNSUPPORTED = -2  # MGP_EUNSUPPORTED
LIMIT_LDS = {("float64", 3): 163728, ("float64", 2): 161200, ("float32", 3): 161552, ("float32", 2): 163392}
KOUT = O.kout(S.LENGTH_SCALE)


def _dt(dtype):
    return getattr(torch, dtype)


def _dev(x, dtype=None):
    t = torch.as_tensor(np.array(x, order="C"), device=DEV)  # (a C-ordered copy: the shared cases are read-only)
    return t.to(_dt(dtype)) if dtype is not None else t


def _np(t):
    return t.double().cpu().numpy()


def _held(got, ref, dtype, t64, e_cal, F, what, scale_of=None):
    """Assert ``got`` against ``ref``: t64 at fp64, the calibrated bound at fp32.  ``scale_of``: the array whose
    size the bound is taken from when ``ref`` is a cancelled difference of it."""
    base = ref if scale_of is None else scale_of
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.all(np.isfinite(got)), f"{what}: not finite"
    rms = float(np.sqrt(np.mean(base**2))) if base.size else 0.0
    den = np.abs(base) + rms
    err = float(np.max(np.abs(got - ref) / np.where(den > 0, den, 1.0))) if ref.size else 0.0
    if dtype == "float64":
        bound = t64
        print(f"{what}: fp64 error {err:.2e} (bound {bound:.0e})")
    else:
        floor = max(e_cal, S.FP32_FLOOR)
        bound = min(F * floor, 1e-3)
        print(f"RATIO {what}: fp32 error {err:.2e}, plain fp32 {e_cal:.2e}, ratio {err / floor:.2f}")
    assert err <= bound, f"{what}: error {err:.3e} above {bound:.3e}"


_TABLES = {}


def _tables(dtype):
    """The device copies of the problem, per dtype: features, the combined query table, the response table as the
    observed columns alone and inside wider tables whose other columns are NaN."""
    if dtype not in _TABLES:
        P = S.problem()
        wide = np.full((len(P.Y), 5), np.nan)
        wide[:, 1:4] = P.Y
        y3 = _dev(P.Y, dtype)
        _TABLES[dtype] = dict(X=_dev(P.X, dtype), FQ=_dev(P.FQ, dtype), Y3=y3, Y2=y3[:, 1:].contiguous(),
                              wide=_dev(wide, dtype))
    return _TABLES[dtype]


def _posterior(c, dtype, form, nn=None):
    """One mgp_shear_posterior_* call through the C ABI: (rc, mean, kk, ykinvy, info, (grid, lds), kernel name)."""
    from muygpys_amd import _lib

    dt, T = _dt(dtype), _tables(dtype)
    nn = c.nn if nn is None else nn
    b, k = nn.shape
    i = c.in_count
    bi, ni = _dev(c.bi), _dev(nn)
    fq, bptr = T["FQ"], _lib.ptr(bi)
    table = T["Y3"] if i == 3 else T["Y2"]
    tg, off, stride, batch = table, 0, i, 0
    if form == "gathered":
        comp = list(range(3 - i, 3))
        tg = _dev(np.swapaxes(c.Y[nn][:, :, comp], -2, -1), dtype)
        assert tuple(tg.shape) == (b, i, k) and tg.is_contiguous()
        stride, batch = 0, 1
    elif form == "strided":  # the Y[:, 1:] view of the 3-column table (2-in); columns 1..3 of a 5-column one (3-in)
        tg, off, stride = (T["Y3"], 1, 3) if i == 2 else (T["wide"], 1, 5)
    elif form == "rows":  # batch_idx == NULL: the query of neighbourhood nb is row nb of the query table
        fq, bptr = T["FQ"][bi].contiguous(), None
    else:
        assert form == "table"
    out = [torch.full(s, float("nan"), device=DEV, dtype=dt) for s in ((b, 3), (b, 3, 3), (b,))]
    info = torch.zeros(1, device=DEV, dtype=torch.int32)
    mode = _lib.SHEAR_NOISE_33 if c.mode == "shear33" else _lib.SHEAR_NOISE_HOMOSCEDASTIC
    rc = _lib.fn("shear_posterior", dt)(
        _lib.ptr(fq), _lib.ptr(T["X"]), bptr, _lib.ptr(ni), b, k, i,
        _lib.C.c_void_p(tg.data_ptr() + off * tg.element_size()), stride, batch, float(c.ell), mode, float(c.eps),
        *(_lib.ptr(t) for t in out), _lib.ptr(info), _lib.stream_ptr(),
    )
    torch.cuda.synchronize()
    if rc != 0:
        return rc, None, None, None, None, None, None
    return rc, out[0], out[1], out[2], int(info.item()), _lib.last_launch_geometry(), _lib.last_kernel()


def _posterior_cases():
    return [pytest.param(dtype, *c, id=f"{dtype}-in{c[0]}-{c[1]}-k{c[2]}-b{c[3]}") for dtype in DTYPES
            for c in S.sweep(dtype)]


@pytest.mark.parametrize("dtype,in_count,mode,k,b", _posterior_cases())
def test_a_fused_posterior_through_the_abi(dtype, in_count, mode, k, b):
    c = S.case(in_count, mode, k, b)
    cal = S.calibration(in_count, mode, k, b) if dtype == "float32" else (0.0, 0.0, 0.0)
    what = f"posterior {dtype} in={in_count} {mode} k={k} b={b}"
    runs = {form: _posterior(c, dtype, form) for form in ("table", "gathered", "strided", "rows")}
    for form, (rc, mean, kk, yk, info, geom, name) in runs.items():
        assert rc == 0 and info == 0, (form, rc, info)
        assert name == f"mgp::shear_posterior_kernel<{'float' if dtype == 'float32' else 'double'},{in_count}>"
        assert all(bool(torch.isfinite(t).all()) for t in (mean, kk, yk)), form
    _, mean, kk, yk, _, (grid, lds), _ = runs["table"]
    for form in ("gathered", "strided", "rows"):
        for got, ref, out in zip(runs[form][1:4], (mean, kk, yk), ("mean", "kk", "ykinvy")):
            assert torch.equal(got, ref), f"{what}: {out} of the {form} form differs from the table form"
        assert runs[form][5] == (grid, lds)
    # the launch: a persistent grid (a workgroup takes a second neighbourhood when b is above it), the LDS request
    assert grid == min(b, 256 * min(16, (160 * 1024) // (-(-lds // 1280) * 1280)))
    if b in (S.REUSE_B, 300):
        assert grid < b, (grid, b)
    lo, hi = S.PAIR_64K[dtype, in_count]
    if k == lo:
        assert lds <= 65536, lds
    if k == hi:
        assert lds > 65536, lds
    if k == S.LIMIT[dtype, in_count]:
        assert lds == LIMIT_LDS[dtype, in_count] <= 160 * 1024
    _held(_np(mean), c.mean, dtype, 1e-9, cal[0], F_POSTERIOR, what + " mean")
    _held(_np(kk), c.kk, dtype, 1e-9, cal[1], F_POSTERIOR, what + " kk")
    _held(_np(yk), c.ykinvy, dtype, 1e-9, cal[2], F_POSTERIOR, what + " ykinvy")
    _held(KOUT - _np(kk), KOUT - c.kk, dtype, 1e-9, cal[1], F_POSTERIOR, what + " Kout - kk", scale_of=c.kk)
    np.testing.assert_array_equal(_np(kk), np.swapaxes(_np(kk), 1, 2))  # both triangles are written from one sum


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("in_count", [3, 2])
def test_b_capacity_is_what_the_library_reports(dtype, in_count):
    from muygpys_amd import _lib

    limit = S.LIMIT[dtype, in_count]
    assert _lib.shear_max_nn_count(_dt(dtype), in_count) == limit
    mode = S.noise_modes(in_count)[0]
    c = S.case(in_count, mode, limit, 1)
    over = np.ascontiguousarray(S.problem().order[c.bi, :limit + 1]).astype(np.int64)
    assert _posterior(c, dtype, "table", nn=over)[0] == UNSUPPORTED
    # ... and through MuyGPS: the ValueError that names the limit
    T = _tables(dtype)
    m = _model(in_count, mode, c.ell, c.eps)
    cross, pair, nn_t = m.make_predict_tensors(torch.arange(1, device=DEV), _dev(over), T["FQ"][_dev(c.bi)], T["X"],
                                               T["Y3"] if in_count == 3 else T["Y2"])
    with pytest.raises(ValueError, match=f"nn_count <= {limit} "):
        m.posterior_mean(m.kernel(pair), m.kernel(cross), nn_t.swapaxes(-2, -1))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("in_count,mode", [(3, "shear33"), (3, "homoscedastic"), (2, "homoscedastic")])
def test_c_singular_neighbourhoods_on_a_reused_workgroup(dtype, in_count, mode):
    """Without a nugget a duplicated neighbour makes K singular: NaN in that row's outputs and a count in ``info``,
    nothing else disturbed -- also when the workgroup goes on to (or comes from) another neighbourhood."""
    c = S.case(in_count, mode, 3, S.REUSE_B, 0.0)
    bad = [0, 5, 4096 + 3]
    nn = c.nn.copy()
    nn[bad, 1] = nn[bad, 0]
    rc, mean, kk, yk, info, (grid, _), _ = _posterior(c, dtype, "table", nn=nn)
    assert rc == 0 and grid == 4096 < c.b
    assert info == 3
    good = np.ones(c.b, dtype=bool)
    good[bad] = False
    for t in (mean, kk, yk):
        nan_rows = torch.isnan(t).reshape(c.b, -1)
        assert bool(nan_rows[_dev(~good)].all()) and not bool(nan_rows[_dev(good)].any())
    cal = S.calibration(in_count, mode, 3, S.REUSE_B, 0.0) if dtype == "float32" else (0.0, 0.0, 0.0)
    what = f"singular {dtype} in={in_count} {mode}"
    # (the calibration covers all rows, the comparison the healthy ones: both are maxima over nearly the same set)
    _held(_np(mean)[good], c.mean[good], dtype, 1e-9, cal[0], F_POSTERIOR, what + " mean")
    _held(_np(kk)[good], c.kk[good], dtype, 1e-9, cal[1], F_POSTERIOR, what + " kk")
    _held(_np(yk)[good], c.ykinvy[good], dtype, 1e-9, cal[2], F_POSTERIOR, what + " ykinvy")


# ---------------------------------------------------------------------------------------------------------------------
# the materialised multi-output solve


def _solve(s, dtype, K=None, want=(True, True, True)):
    """mgp_solve_multi_* through the C ABI: (rc, mean (b, m, R), kk (b, m, m), ykinvy (b, R), info, geometry)."""
    from muygpys_amd import _lib

    dt = _dt(dtype)
    b, n, m = s.Kc.shape
    R = s.Y.shape[2]
    Kd, Kc, Y = _dev(s.K if K is None else K, dtype), _dev(s.Kc, dtype), _dev(s.Y, dtype)
    out = [torch.full(shape, float("nan"), device=DEV, dtype=dt) if w else None
           for shape, w in zip(((b, m, R), (b, m, m), (b, R)), want)]
    info = torch.zeros(1, device=DEV, dtype=torch.int32)
    rc = _lib.fn("solve_multi", dt)(_lib.ptr(Kd), _lib.ptr(Kc), _lib.ptr(Y) if R else None, b, n, m, R,
                                    *(_lib.ptr(t) for t in out), _lib.ptr(info), _lib.stream_ptr())
    torch.cuda.synchronize()
    if rc != 0:
        return rc, None, None, None, None, None
    assert "solve_multi_kernel" in _lib.last_kernel()
    return rc, out[0], out[1], out[2], int(info.item()), _lib.last_launch_geometry()


def _solve_held(s, dtype, mean, kk, yk, what):
    cal = S.solve_in_dtype(s.K, s.Kc, s.Y, np.float32) if dtype == "float32" else (s.mean, s.kk, s.ykinvy)
    for got, ref, c32, out in zip((mean, kk, yk), (s.mean, s.kk, s.ykinvy), cal, ("mean", "kk", "ykinvy")):
        if got is None:
            continue
        _held(_np(got), ref, dtype, 1e-12, S.metric_error(c32, ref), F_SOLVE, f"{what} {out}")


SOLVE_SHAPES = [(1, 1, 0), (1, 1, 1), (2, 3, 1), (3, 1, 2), (5, 2, 0), (6, 3, 1), (7, 5, 4), (13, 3, 16), (60, 3, 1),
                (61, 3, 1)]


def _solve_cases():
    out = []
    for dtype in DTYPES:
        out += [(dtype, 37, *shape) for shape in SOLVE_SHAPES]
        out += [(dtype, S.REUSE_B, 5, 2, 0), (dtype, S.REUSE_B, 5, 2, 3), (dtype, 37, S.SOLVE_LIMIT[dtype], 3, 1),
                (dtype, 300, S.SOLVE_LIMIT[dtype], 3, 1)]
    return [pytest.param(*c, id="-".join(str(v) for v in c)) for c in out]


@pytest.mark.parametrize("dtype,b,n,m,R", _solve_cases())
def test_d_solve_multi_through_the_abi(dtype, b, n, m, R):
    s = S.spd_systems(b, n, m, R)
    want = (R > 0, True, R > 0)  # (without responses the ABI takes no mean / ykinvy pointer)
    rc, mean, kk, yk, info, (grid, lds) = _solve(s, dtype, want=want)
    assert rc == 0 and info == 0
    if b > 256 * 16 or (b == 300 and n == S.SOLVE_LIMIT[dtype]):
        assert grid < b, (grid, b)  # workgroups take a second system
    if n == S.SOLVE_LIMIT[dtype]:
        assert 150 * 1024 < lds <= 160 * 1024, lds
    _solve_held(s, dtype, mean, kk, yk, f"solve_multi {dtype} b={b} n={n} m={m} R={R}")
    np.testing.assert_array_equal(_np(kk), np.swapaxes(_np(kk), 1, 2))


@pytest.mark.parametrize("dtype", DTYPES)
def test_d_solve_multi_capacity(dtype):
    """The largest n with (m, R) = (3, 1) is what the sizing formula gives; n + 1 is refused, not launched."""
    n = S.SOLVE_LIMIT[dtype]
    assert _solve(S.spd_systems(2, n, 3, 1), dtype)[0] == 0
    assert _solve(S.spd_systems(2, n + 1, 3, 1), dtype)[0] == UNSUPPORTED


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,m,R", [(7, 5, 4), (13, 3, 16), (61, 3, 1)])
def test_d_solve_multi_reads_the_lower_triangle_and_honours_null_outputs(dtype, n, m, R):
    s = S.spd_systems(37, n, m, R)
    _, mean, kk, yk, info, _ = _solve(s, dtype)
    assert info == 0
    upper = np.triu(np.ones((n, n), dtype=bool), 1)
    rc, *lower, info, _ = _solve(s, dtype, K=np.where(upper, np.nan, s.K))
    assert rc == 0 and info == 0
    for got, ref in zip(lower, (mean, kk, yk)):
        assert torch.equal(got, ref), "NaN above the diagonal of Kin changes the outputs"
    for drop in range(3):
        want = tuple(j != drop for j in range(3))
        rc, *outs, info, _ = _solve(s, dtype, want=want)
        assert rc == 0 and info == 0 and outs[drop] is None
        for j, ref in enumerate((mean, kk, yk)):
            assert j == drop or torch.equal(outs[j], ref), (drop, j)


# ---------------------------------------------------------------------------------------------------------------------
# the block tensors

_VARIANTS = {"33": ((0, 1, 2), (0, 1, 2)), "kin23": ((1, 2), (1, 2)), "kcross23": ((1, 2), (0, 1, 2))}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("variant", list(_VARIANTS))
@pytest.mark.parametrize("G,n,m", [(1, 1, 1), (3, 5, 7), (257, 4, 1), (2, 33, 33), (1000, 3, 1)])
def test_e_shear_tensor(dtype, variant, G, n, m):
    from muygpys_amd import _lib
    from muygpys_amd._src.gp.kernels.shear import hip as K

    ell = 1.3
    rng = np.random.default_rng([S.SEED, G, n, m])
    r, phi = 4.0 * np.sqrt(rng.uniform(0, 1, (G, n, m))), rng.uniform(0, 2 * np.pi, (G, n, m))
    diffs = np.stack([r * np.cos(phi), r * np.sin(phi)], -1)  # |d|^2 <= 16
    rows, cols = _VARIANTS[variant]
    B = O.block(diffs[..., 0], diffs[..., 1], ell)[..., list(rows), :][..., list(cols)]
    ref = np.moveaxis(B, (-2, -1), (-4, -2))  # shear_oracle.tensor without its squeeze: (G, I, n, O, m)
    code = {"33": _lib.SHEAR_33, "kin23": _lib.SHEAR_KIN23, "kcross23": _lib.SHEAR_KCROSS23}[variant]
    got = K._tensor(_dev(diffs, dtype), code, ell)
    assert got.dtype == _dt(dtype) and got.numel() == ref.size
    assert tuple(got.shape) == tuple(v for v in ref.shape if v != 1)
    e_cal = S.metric_error(S.tensor_in_dtype(diffs, ell, rows, cols, np.float32), ref) if dtype == "float32" else 0.0
    _held(_np(got).reshape(ref.shape), ref, dtype, 1e-12, e_cal, F_TENSOR, f"shear_tensor {dtype} {variant} {G, n, m}")


# ---------------------------------------------------------------------------------------------------------------------
# through MuyGPS


def _model(in_count, mode, ell, eps):
    from muygpys_amd.gp.deformation import F2, DifferenceIsotropy
    from muygpys_amd.gp.hyperparameter import FixedScale, ScalarParam
    from muygpys_amd.gp.kernels import ShearKernel, ShearKernel2in3out
    from muygpys_amd.gp.muygps import MuyGPS
    from muygpys_amd.gp.noise import HomoscedasticNoise, ShearNoise33

    dfm = DifferenceIsotropy(F2, length_scale=ScalarParam(ell))
    kernel = ShearKernel(deformation=dfm) if in_count == 3 else ShearKernel2in3out(deformation=dfm)
    noise = ShearNoise33(eps) if mode == "shear33" else HomoscedasticNoise(eps)
    return MuyGPS(kernel=kernel, noise=noise, scale=FixedScale())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("in_count,mode,k", [(3, "shear33", 3), (3, "shear33", 5), (2, "homoscedastic", 5)])
def test_f_partial_blocks_and_the_strided_table_through_muygps(dtype, in_count, mode, k, monkeypatch):
    """n = 9 (n % 4 = 1), n = 15 (n % 4 = 3), and the 2-in model handed the non-contiguous Y[:, 1:] view of the
    3-column table, which the launch must read in place with its row stride of 3."""
    from muygpys_amd import _lib, lazy, lazy_eval

    c = S.case(in_count, mode, k, 37)
    T = _tables(dtype)
    table = T["Y3"] if in_count == 3 else T["Y3"][:, 1:]
    assert in_count == 3 or not table.is_contiguous()
    strides = []
    real = lazy_eval._shear_launch
    monkeypatch.setattr(lazy_eval, "_shear_launch", lambda *a: strides.append((a[2].data_ptr(), a[3])) or real(*a))
    m = _model(in_count, mode, c.ell, c.eps)
    cross, pair, nn_t = m.make_predict_tensors(torch.arange(c.b, device=DEV), _dev(c.nn), T["FQ"][_dev(c.bi)], T["X"],
                                               table)
    nn_t = nn_t.swapaxes(-2, -1)
    assert isinstance(nn_t, lazy.LazyTargets)
    Kin, Kc = m.kernel(pair), m.kernel(cross)
    mean = m.posterior_mean(Kin, Kc, nn_t)
    assert "shear_posterior_kernel" in _lib.last_kernel()
    var = m.posterior_variance(Kin, Kc)
    assert strides == [(table.data_ptr(), 3)], "one launch, on the caller's table, with its stride"
    cal = S.calibration(in_count, mode, k, 37) if dtype == "float32" else (0.0, 0.0, 0.0)
    what = f"MuyGPS {dtype} in={in_count} k={k}"
    _held(_np(mean), c.mean, dtype, 1e-9, cal[0], F_POSTERIOR, what + " mean")
    _held(_np(var), KOUT - c.kk, dtype, 1e-9, cal[1], F_POSTERIOR, what + " covariance", scale_of=c.kk)
