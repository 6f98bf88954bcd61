"""GPU: the argument modes of the fused posterior -- the three noise layouts, ``batch_idx`` or None, a query table of its
own, table or gathered responses, the non-SPD flag -- in every kernel family behind the dispatcher (the run-time-shape
wave kernels, the built-in static shapes, fused_rhs in its five forms, fused_rhs_mf, fused_wide, fused_wide64,
fused_generic; plain and prepared tables) against the numpy fp64 restatement of the oracle in tests/posterior_cases.py.

Every call goes through ``muygpys_amd.fused.posterior_mean_var`` with an explicit ``path`` and ``packed`` and asserts, in
this order, the kernel that served it (``_lib.last_kernel()``), ``info`` and the outputs.  The band is RTOL of
tests/util.py (fp64 1e-5, fp32 1e-3): ``assert_close`` for the mean, the pure relative ``assert_rel_close`` for the
variance and y^T K^-1 y.  No case uses the calibration allowance of ``assert_rel_close`` (CALIBRATED is empty): the
largest errors measured on an MI355X, as shares of the band, are 9.1e-3 (mean), 1.3e-2 (variance) and 2.2e-3 (ykinvy)
in fp32 and 1.9e-9, 1.2e-8 and 4.9e-10 in fp64.

Four tests: every case of the sample (248: 38 per wave family and dtype, 38 / 20 fused_rhs fp32 / fp64, 14
fused_rhs_mf, 22 per static family, 20 fused_wide, 20 fused_wide64, 8 per generic family); one launch of 20011
neighbourhoods per family, whose workgroups all come round a second time; the non-SPD flag and the bit-for-bit
agreement of the modes, once per entry of the family table.

What the inputs must be for these bands to be a fair demand, and for a wrong mode to leave them, is asserted on the CPU
in tests/test_posterior_cases_cpu.py."""

import numpy as np
import pytest
import torch

from tests import posterior_cases as PC
from tests.util import RTOL, assert_close, assert_rel_close, to_dev

pytestmark = pytest.mark.gpu

TORCH = {"float32": torch.float32, "float64": torch.float64}
# cases that need the calibration allowance (the fp32 restatement of the same case): {case id: measured error}
CALIBRATED = {}


def _table(x, t, off):
    """A device table; ``off``: its base one element off the 16-byte grid (a flat allocation of one element more)."""
    x = to_dev(x, t)
    if not off:
        assert x.data_ptr() % 16 == 0
        return x
    flat = torch.empty(x.numel() + 1, dtype=t, device="cuda")
    flat[1:] = x.reshape(-1)
    view = flat[1:].view(x.shape)
    assert view.data_ptr() % 16 == x.element_size() and view.is_contiguous()
    return view


def _launch(c, P, noise=None, gathered=None, bi=None, noise_rows=None):
    """One call of the case (``noise`` / ``gathered`` / ``bi``: another form of the same numbers than the case's own)
    -> (kernel name, info, mean (b, R), var (b,), ykinvy (b, R) or None) as numpy."""
    from muygpys_amd import _lib
    from muygpys_amd.fused import KernelSpec, posterior_mean_var

    t = TORCH[c["dtype"]]
    noise = c["noise"] if noise is None else noise
    gathered = c["gathered"] if gathered is None else gathered
    bi = c["bi"] if bi is None else bi
    Xn = _table(P.Xn, t, c["off"])
    Xq = _table(P.Xq, t, c["off"]) if c["own_query"] else Xn
    ni = to_dev(P.ni)
    Y = to_dev(P.Y, t)
    rows = P.noise_rows if noise_rows is None else noise_rows
    d_noise = {"scalar": PC.NOISE, "table": to_dev(P.table, t), "batch": to_dev(rows, t)}[noise]
    spec = KernelSpec(c["kernel"], c["metric"], list(P.ls) if c["aniso"] else P.ls, d_noise)
    info = torch.zeros(1, dtype=torch.int32, device="cuda")
    out = posterior_mean_var(spec, Xq, Xn, to_dev(P.bi) if bi else None, ni, Y[ni] if gathered else Y, want_ykinvy=c["yk"],
                             info=info, path=c["path"], packed=c["packed"], gathered=gathered)
    name = _lib.last_kernel()
    torch.cuda.synchronize()
    mean, var = out[0].cpu().numpy().reshape(P.b, c["R"]), out[1].cpu().numpy()
    yk = out[2].cpu().numpy().reshape(P.b, c["R"]) if c["yk"] else None
    return name, int(info.item()), mean, var, yk


def _served_by(c, name, any_wave=False):
    if any_wave and c["family"].startswith("wave"):
        assert name.startswith("mgp::fused_wave_kernel<"), name
    elif c["exact"]:
        assert name == c["prefix"], (name, c["prefix"])
    else:
        assert name.startswith(c["prefix"]), (name, c["prefix"])
    if c["packed"]:  # the packed flag of the wave kernels / the suffix of fused_rhs_mf
        assert ",true,false,true," in name or name.endswith("[prepared tables]"), name
    else:  # (the prefix of a plain wave entry ends with the packed flag: false)
        assert "[prepared tables]" not in name, name


def _held(c, got, ref, rows=None):
    """mean, var and (where requested) ykinvy against the fp64 restatement, each figure printed before it is held."""
    rtol = RTOL[c["dtype"]]
    mean, var, yk = got
    m_ref, v_ref, y_ref = ref
    figures = [PC.band_error(mean, m_ref), PC.rel_error(var, v_ref), PC.rel_error(yk, y_ref) if yk is not None else 0.0]
    print(f"FIGURES {c['id']} {c['dtype']} mean {figures[0] / rtol:.2e} var {figures[1] / rtol:.2e} ykinvy {figures[2] / rtol:.2e} of the band")
    cal = (None, None)
    if c["id"] in CALIBRATED:
        _, v32, y32 = PC.outputs(c, np.float32, rows=rows)
        cal = (v32, y32)
    assert_close(mean, m_ref, rtol, f"{c['id']}: mean")
    assert_rel_close(var, v_ref, rtol, f"{c['id']}: var", calibration=cal[0])
    if yk is not None:
        assert_rel_close(yk, y_ref, rtol, f"{c['id']}: ykinvy", calibration=cal[1])


# ---- 1. the modes ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", [c["id"] for c in PC.CASES])
def test_modes(cid):
    c, P = PC.BY_ID[cid], PC.problem(cid)
    name, info, mean, var, yk = _launch(c, P)
    _served_by(c, name)
    assert info == 0
    _held(c, (mean, var, yk), PC.reference(cid))


# ---- 2. the second pass of the persistent loop -------------------------------------------------------------------------
@pytest.mark.parametrize("cid", [c["id"] for c in PC.LONG_CASES])
def test_second_pass_of_the_persistent_loop(cid):
    from muygpys_amd import _lib

    c, P = PC.BY_ID[cid], PC.long_problem(cid)
    b = c["b"]
    name, info, mean, var, yk = _launch(c, P)
    workgroups, _ = _lib.last_launch_geometry()
    _served_by(c, name, any_wave=True)
    assert info == 0
    # neighbourhoods per task: 64 / NP in the wave kernels, two in the folded rhs variant, one otherwise
    per_task = 64 // int(name.split("<")[1].split(",")[1]) if "fused_wave_kernel" in name else (2 if ",fold>" in name else 1)
    print(f"{cid}: {name}, {workgroups} workgroups, {per_task} neighbourhood(s) per task")
    assert workgroups >= 1 and workgroups * per_task * 2 <= b, (workgroups, per_task)
    rng = np.random.default_rng(b)
    first_pass = workgroups * per_task
    # 64 rows: the ends, 20 of the first pass (as far as it has that many), the rest of the later passes
    early = rng.choice(np.arange(2, first_pass), size=min(20, first_pass - 2), replace=False) if first_pass > 2 else np.array([], dtype=np.int64)
    late = rng.choice(np.arange(max(first_pass, 2), b - 2), size=60 - len(early), replace=False)
    picked = np.unique(np.concatenate([[0, 1, b - 2, b - 1], early, late]))
    assert len(picked) == 64 and (picked >= first_pass).sum() >= 42
    ref = PC.outputs(c, np.float64, rows=picked)
    _held(c, (mean[picked], var[picked], None if yk is None else yk[picked]), ref, rows=picked)


# ---- 3. the non-SPD flag -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", [c["id"] for c in PC.ENTRY_CASES])
def test_non_spd_flag(cid):
    """Three neighbourhoods with a noise entry of -2.0 -- at the first, the middle and the last neighbour: a strictly
    negative pivot, no rounding-dependent zero -- are counted in ``info`` and NaN in every output; the other 34 are
    untouched."""
    c, P = PC.BY_ID[cid], PC.problem(cid)
    k = c["k"]
    bad = np.array(PC.BAD_ROWS)
    noise = np.array(P.noise_rows)
    noise[bad, [0, k // 2, k - 1]] = -2.0
    good = np.setdiff1d(np.arange(P.b), bad)
    name, info, mean, var, yk = _launch(c, P, noise_rows=noise)
    _served_by(c, name)
    assert info == 3
    for out, what in ((mean, "mean"), (var[:, None], "var"), (yk, "ykinvy")):
        if out is not None:
            assert np.array_equal(np.isnan(out).any(axis=1), np.isin(np.arange(P.b), bad)), (what, np.flatnonzero(np.isnan(out).any(axis=1)))
            assert np.isnan(out[bad]).all(), what
    ref = tuple(r[good] for r in PC.reference(cid))
    _held(c, (mean[good], var[good], None if yk is None else yk[good]), ref, rows=good)


# ---- 4. the modes agree bit for bit ------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", [c["id"] for c in PC.ENTRY_CASES])
def test_modes_agree_bit_for_bit(cid):
    """The same numbers through other pointers -- the noise table against batch noise built as table[nn_idx], table
    responses against gathered ones built as Y[nn_idx], ``batch_idx = arange(b)`` against None -- reach the same
    kernel and the same arithmetic in the same order: identical bits.  (fused_rhs_mf on prepared tables takes no
    gathered responses through posterior_mean_var: that pair is run on its plain form.)"""
    c, P = PC.BY_ID[cid], PC.problem(cid)
    assert c["noise"] == "batch" and not c["gathered"] and not c["bi"] and np.array_equal(P.bi, np.arange(P.b))
    base = _launch(c, P)
    _served_by(c, base[0])
    assert base[1] == 0
    others = {"noise table": dict(noise="table"), "batch_idx = arange(b)": dict(bi=True)}
    if c["can_gather"]:
        others["gathered responses"] = dict(gathered=True)
    for what, form in others.items():
        got = _launch(c, P, **form)
        assert got[0] == base[0], (what, got[0], base[0])
        assert got[1] == 0
        for a, g, out in zip(base[2:], got[2:], ("mean", "var", "ykinvy")):
            if a is not None:
                assert a.tobytes() == g.tobytes(), (what, out, float(np.abs(a.astype(np.float64) - g).max()))
