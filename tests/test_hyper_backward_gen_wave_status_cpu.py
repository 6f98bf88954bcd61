"""CPU: the wave-sized hyper-parameter backward of the general-smoothness Matern (mgp_hyper_backward_gen_wave_*;
include/muygpys_hip.h) -- the status of every refused or empty call, decided BEFORE any HIP call and in the order the
header states; its parameter list against mgp_hyper_backward_gen_large_*'s; the compiler's register record of every
instantiation that is built; the environment switch.

One rule is violated per row, starting from arguments that would launch.  Host buffers stand in for device pointers:
nothing dereferences them before the status is decided.  No row here reaches a launch."""

import ctypes as C
import json
import os
import re
import subprocess
import sys

import pytest

from muygpys_amd import _abi, _lib

OK, EINVAL, EUNSUPPORTED = 0, -1, -2
INT_MAX = 2**31 - 1

NAMES = "feat d bi ni b k tg R nm eps nd nu mid ls lsc gm gv gyk gls gnz gnu info st".split()
NUMBERS = dict(d=4, b=3, k=5, R=1, nm=0, eps=1e-3, nu=1.3, mid=0, lsc=1)
OPTIONAL = ("nd", "st")
OUTPUTS = {n: None for n in ("gls", "gnz", "gnu")}
COTANGENTS = {n: None for n in ("gm", "gv", "gyk")}
NOTHING = {n: None for n in NAMES if n not in NUMBERS}
BUF = (C.c_double * 64)()
PTR = C.addressof(BUF)
NAN = float("nan")


def status(suf, **changes):
    args = {n: NUMBERS[n] if n in NUMBERS else (None if n in OPTIONAL else PTR) for n in NAMES}
    assert set(changes) <= set(NAMES)
    args.update(changes)
    return getattr(_lib.load(), f"mgp_hyper_backward_gen_wave_{suf}")(*[args[n] for n in NAMES])


GRID = [
    # 1. sizes, and a smoothness that is not > 0
    ("b < 0", dict(b=-1), EINVAL), ("k < 1", dict(k=0), EINVAL), ("d < 1", dict(d=0), EINVAL), ("R < 1", dict(R=0), EINVAL),
    ("nu = 0", dict(nu=0.0), EINVAL), ("nu NaN", dict(nu=NAN), EINVAL),
    # 2. the empty batch: nothing else is looked at -- but the sizes and the smoothness's sign are
    ("empty batch, all pointers NULL", dict(b=0, **NOTHING), OK),
    ("empty batch, wild ids", dict(b=0, **NOTHING, mid=7, nm=8, lsc=9), OK),
    ("empty batch, shapes beyond the kernel", dict(b=0, k=5000, d=900, nu=31.0, **NOTHING), OK),
    ("empty batch, k < 1", dict(b=0, k=0), EINVAL), ("empty batch, nu NaN", dict(b=0, nu=NAN), EINVAL),
    # 3. pointers, cotangents, outputs, ids
    *[(f"{p} NULL", {p: None}, EINVAL) for p in ("feat", "ni", "tg", "ls")],
    ("all three cotangents NULL", COTANGENTS, EINVAL), ("all three outputs NULL", OUTPUTS, EINVAL),
    ("grad_ykinvy with R = 3", dict(R=3), EINVAL),
    *[(f"metric id {i}", dict(mid=i), EINVAL) for i in (-1, 2)], *[(f"noise mode {i}", dict(nm=i), EINVAL) for i in (-1, 3)],
    *[(f"noise mode {i} without noise_dev", dict(nm=i, nd=None), EINVAL) for i in (1, 2)],
    *[(f"ls_count {i} at d = 4", dict(lsc=i), EINVAL) for i in (0, 2, 5)],
    # 4. ... and only then what the kernel does not serve
    ("nu = 30.5", dict(nu=30.5), EUNSUPPORTED), ("nu = inf", dict(nu=float("inf")), EUNSUPPORTED),
    ("nu = 30.5, outputs NULL", dict(nu=30.5, **OUTPUTS), EINVAL), ("nu = 30.5, metric id 2", dict(nu=30.5, mid=2), EINVAL),
    ("k + 2 = 65", dict(k=63), EUNSUPPORTED), ("k + 2 = 65, cotangents NULL", dict(k=63, **COTANGENTS), EINVAL),
    ("k = INT_MAX", dict(k=INT_MAX), EUNSUPPORTED), ("k = INT_MAX - 1", dict(k=INT_MAX - 1), EUNSUPPORTED),
    ("d = 65", dict(d=65), EUNSUPPORTED), ("d = 65, ls NULL", dict(d=65, ls=None), EINVAL),
]


@pytest.mark.parametrize("suf", ["f32", "f64"])
@pytest.mark.parametrize("name, changes, want", GRID, ids=[n for n, _, _ in GRID])
def test_status_of_refused_and_empty_calls(name, changes, want, suf):
    assert status(suf, **changes) == want


def test_fp64_feature_counts_beyond_the_instantiations_are_refused():
    assert status("f64", d=17) == EUNSUPPORTED           # up to 32 slots: d <= 16
    assert status("f64", d=9, k=31) == EUNSUPPORTED      # beyond: d <= 8


def test_parameter_list_is_the_slab_entry_without_its_workspace():
    text = " ".join(open(_abi.HEADER).read().split())

    def params(name):
        return [p.strip() for p in re.search(rf"int {name}\(([^)]*)\);", text).group(1).split(",")]

    for suf in ("f32", "f64"):
        slab = params(f"mgp_hyper_backward_gen_large_{suf}")
        assert slab[-3:-1] == ["void* workspace", "int64_t workspace_bytes"]
        assert params(f"mgp_hyper_backward_gen_wave_{suf}") == slab[:-3] + slab[-1:]


def test_no_spills_no_scratch():
    with open(os.path.join(os.path.dirname(_lib.LIB_PATH), "kernel_resources.json")) as f:
        res = json.load(f)
    mine = {n: r for n, r in res.items() if "gen_wave_backward_kernel" in n}
    assert len(mine) >= 8, sorted(mine)
    for name, r in mine.items():
        assert r["VGPRs Spill"] == 0 and r["ScratchSize [bytes/lane]"] == 0, (name, r)


def test_an_invalid_mode_in_the_environment_fails_at_import_naming_the_value():
    env = dict(os.environ, MUYGPYS_HIP_GEN_BACKWARD="wave")
    r = subprocess.run([sys.executable, "-c", "import muygpys_amd.fused"], env=env, capture_output=True, text=True,
                       cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert r.returncode != 0 and "MUYGPYS_HIP_GEN_BACKWARD='wave'" in r.stderr, r.stderr
    env["MUYGPYS_HIP_GEN_BACKWARD"] = "wavefront"
    code = "import muygpys_amd.fused as f; assert f.gen_backward_default() == 'wavefront'"
    assert subprocess.run([sys.executable, "-c", code], env=env, cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__)))).returncode == 0
