"""GPU: the fused backward up to mgp_max_nn_count_backward, every kernel rung against the fp64 vector-Jacobian product
at its edges -- F, the backward instantiation of the forward wave kernel (dealt triangle and row per lane, built in
and compiled at run time); W, all 28 instantiations of backward_wave_kernel; L, the LDS workgroup kernel at every
thread count, on the single-wave path and with one, two and nine feature chunks.  The cases, the rules that say which
kernel must serve each, and the reference are tests/backward_cases.py; what the inputs must be for the bands below to
be a fair demand is asserted on the CPU in tests/test_backward_cases_cpu.py.

MGP_BACKWARD_DLT and MGP_BACKWARD_LDS are read once per process, so each rung runs in a child of its own
(tests/backward_rung_runner.py: F with neither set, W with MGP_BACKWARD_DLT=0, L with MGP_BACKWARD_LDS=1), one after
another, each under its own time limit; the tests of a rung read the one .npz its child stored.  A child that ends by
signal, abort, time limit or any other failure fails the test that started it, and every remaining test of the
module skips without starting another GPU process.

Every case asserts, in this order: the return code; the name of the kernel that served it against the restated rule
(another kernel is a failure, not a skip); ``info``; then with ``assert_close`` (1e-5 in fp64, 3 x 1e-3 in fp32)
grad_ls and grad_noise PER NEIGHBOURHOOD, unsummed, and the three accumulated tables.  grad_ls and grad_noise start
as NaN and the accumulated tables at 0.25, so an element never written and a store in place of an add both show.
Only F cases of the four shapes compiled on demand may skip, and only where mgp_jit_prepare_backward itself failed.

Measured on an MI355X, the largest error of any case as a share of its band: 0.10 in fp32 (grad_noise of L; 0.028 for
an accumulated table) and 8.4e-8 in fp64.  A library copy whose backward_kernel drops the features of the last chunk
behind its last whole 16-byte piece fails 66 of the 107 L cases."""

import os
import subprocess
import sys

import numpy as np
import pytest

from tests import backward_cases as BC
from tests.backward_rung_runner import FILL
from tests.util import assert_close

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = {"F": {}, "W": {"MGP_BACKWARD_DLT": "0"}, "L": {"MGP_BACKWARD_LDS": "1"}}
# seconds: a few seconds of launches behind the start of the process; F may compile four small shapes
TIME_LIMIT = {"F": 180, "W": 120, "L": 120}
_STATE = {"dead": None, "runs": {}, "skipped": 0}


@pytest.fixture(scope="module")
def rung_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("backward_rungs")


def _results(rung, rung_dir):
    """What the rung's child stored: {case id: {key: array}}; the child is started at the first request."""
    if rung in _STATE["runs"]:
        return _STATE["runs"][rung]
    if _STATE["dead"]:
        pytest.skip(f"no further GPU process after: {_STATE['dead']}")
    out = str(rung_dir / f"{rung}.npz")
    env = {key: v for key, v in os.environ.items() if key not in ("MGP_BACKWARD_DLT", "MGP_BACKWARD_LDS")}
    env.update(ENV[rung])
    cmd = [sys.executable, "-m", "tests.backward_rung_runner", "--rung", rung, "--out", out]
    try:
        r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=TIME_LIMIT[rung])
    except subprocess.TimeoutExpired:
        _STATE["dead"] = f"rung {rung}: no end within {TIME_LIMIT[rung]} s"
        pytest.fail(_STATE["dead"])
    if r.returncode != 0:
        _STATE["dead"] = f"rung {rung}: the child ended with {r.returncode}"
        pytest.fail(_STATE["dead"] + "\n" + r.stderr[-2000:])
    z = np.load(out)
    res = {}
    for i, cid in enumerate(z["ids"]):
        res[str(cid)] = {key.split("/", 1)[1]: z[key] for key in z.files if key.startswith(f"{i}/")}
        res[str(cid)]["index"] = i
    res["__order__"] = [str(cid) for cid in z["ids"]]
    _STATE["runs"][rung] = res
    return res


def _figures(c, got, ref, what):
    print(f"FIGURES {c['id']} {what} {BC.band_error(got, ref) / BC.RTOL[c['dtype']]:.2e} of the band")


@pytest.mark.parametrize("cid", [c["id"] for rung in BC.RUNGS for c in BC.rung_cases(rung)])
def test_case(cid, rung_dir):
    c = BC.BY_ID[cid]
    res = _results(c["rung"], rung_dir)
    got = res[cid]
    rc, info, workgroups, _lds, prep = (int(v) for v in got["meta"])
    name = str(got["name"])
    P = BC.problem(cid)
    if c["expect"] is None:
        # one past the limit: refused, nothing launched (the noted kernel is still the launch before), nothing written
        assert rc == BC.EUNSUPPORTED, rc
        before = res[res["__order__"][got["index"] - 1]]
        assert name == str(before["name"]) and np.array_equal(got["meta"][2:4], before["meta"][2:4]), (name, str(before["name"]))
        assert np.isnan(got["gls"]).all() and np.isnan(got["gnz"]).all()
        assert all((got[key] == FILL).all() for key in ("gnn", "gtg")), "a refused call wrote into an accumulated buffer"
        return
    if prep != 0 and BC.prepared_shape(c) == "demand":
        _STATE["skipped"] += 1
        print(f"SKIPPED so far: {_STATE['skipped']} (mgp_jit_prepare_backward returned {prep})")
        pytest.skip(f"mgp_jit_prepare_backward returned {prep} for a shape compiled on demand")
    assert prep == 0, f"mgp_jit_prepare_backward returned {prep} for a shape that build() prepares"
    assert rc == 0, rc
    assert name == c["expect"], (name, c["expect"])
    rtol = BC.RTOL[c["dtype"]]
    _, ref = BC.reference(cid)
    rows = np.setdiff1d(np.arange(P.b), BC.BAD_ROWS) if c["bad"] else np.arange(P.b)
    if c["bad"]:
        bad = list(BC.BAD_ROWS)
        assert info == 3, info
        # cotangents of a non-SPD neighbourhood are left untouched: the sentinel is still there
        assert np.isnan(got["gls"][bad]).all() and np.isnan(got["gnz"][bad]).all()
    else:
        assert info == 0, info
    if c["b"] == BC.LONG_B:
        print(f"{cid}: {workgroups} workgroups, {c['per_task']} neighbourhood(s) per task")
        assert workgroups >= 1 and workgroups * c["per_task"] < c["b"], (workgroups, c["per_task"])
    compare = []
    if c["want"] != "nn":
        compare += [("gls", got["gls"][rows], ref["gls"]), ("gnz", got["gnz"][rows], ref["gnz"])]
    for key in ("gq", "gnn", "gtg"):
        if key in ref:
            assert key in got, key
            compare.append((key, got[key].astype(np.float64) - FILL, ref[key]))
        else:
            assert key not in got, key
    for what, g, r in compare:
        _figures(c, g, r, what)
    for what, g, r in compare:
        assert_close(g, r, rtol, f"{cid}: {what}")


def test_every_instantiation_is_proven_by_name(rung_dir):
    """All 28 instantiations of backward_wave_kernel, both built-in shapes of F, both of its forms in both slot counts
    and every thread count of L appear among the names the library itself noted after launches that returned 0."""
    names = set()
    for rung in BC.RUNGS:
        res = _results(rung, rung_dir)
        names |= {str(res[cid]["name"]) for cid in res["__order__"] if int(res[cid]["meta"][0]) == 0}
    wave = {n for n in names if n.startswith("mgp::backward_wave_kernel<")}
    assert len(wave) == 28, sorted(wave)
    bwd = "false,backward>"
    assert f"mgp::fused_wave_kernel<float,32,30,1,40,true,false,false,true,{bwd}" in names
    assert f"mgp::fused_wave_kernel<double,64,50,1,8,true,false,false,false,{bwd}" in names
    jit = {n for n in names if n.endswith("backward> [run-time compiled]")}
    for prefix in ("mgp::fused_wave_kernel<float,32,", "mgp::fused_wave_kernel<float,64,", "mgp::fused_wave_kernel<double,32,",
                   "mgp::fused_wave_kernel<double,64,"):
        assert any(n.startswith(prefix) for n in jit), (prefix, sorted(jit))
    for t, threads in (("float", 64), ("float", 128), ("float", 256), ("double", 64), ("double", 128)):
        assert any(n.startswith(f"mgp::backward_kernel<{t}> [threads={threads},") for n in names), (t, threads)
