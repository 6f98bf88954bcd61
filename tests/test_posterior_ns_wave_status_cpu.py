"""CPU: the wave-sized entry with a length scale per neighbourhood (mgp_posterior_ns_wave_*) on the cross-compiled
library -- its parameter list, the status of every refused or empty call in the documented order (null device pointers
stand in: no HIP call is reached), the compiler's record, and the Python switches that are decided without a launch."""

import json
import os
import subprocess
import sys

import pytest

from muygpys_amd import _lib
from tests.test_posterior_ns_status_cpu import EINVAL, EUNSUPPORTED, NUMBERS, OK, OPTIONAL, PTR, REQUIRED

NAMES = "fq fn d bi ni b k tg R tb nm eps nd kid mid lsb lsc mean var yk info st".split()
NOTHING = {n: None for n in NAMES if n not in NUMBERS}
ROWS = [("b < 0", dict(b=-1), EINVAL), ("k < 1", dict(k=0), EINVAL), ("d < 1", dict(d=0), EINVAL), ("R < 1", dict(R=0), EINVAL),
        ("empty batch, nothing looked at", dict(b=0, **NOTHING, kid=99, mid=7, nm=8, lsc=9), OK),
        ("empty batch, k < 1", dict(b=0, k=0), EINVAL),
        *[(f"{p} NULL", {p: None}, EINVAL) for p in REQUIRED.split()],
        *[(f"kernel id {i}", dict(kid=i), EINVAL) for i in (-1, 6)], ("metric id 2", dict(mid=2), EINVAL),
        ("noise mode 3", dict(nm=3), EINVAL), ("table noise without noise_dev", dict(nm=1, nd=None), EINVAL),
        *[(f"ls_count {i} at d = 4", dict(lsc=i), EINVAL) for i in (0, 2, 5)],
        ("the general-nu id", dict(kid=5), EUNSUPPORTED), ("the general-nu id, scales NULL", dict(kid=5, lsb=None), EINVAL),
        ("(b, d) scales", dict(lsc=4), EUNSUPPORTED), ("65 slots", dict(k=63), EUNSUPPORTED),
        ("65 slots by responses", dict(k=50, R=14), EUNSUPPORTED), ("65 slots, scales NULL", dict(k=63, lsb=None), EINVAL),
        ("k = INT_MAX", dict(k=2**31 - 1), EUNSUPPORTED), ("d = 65 / 17", dict(d=(65, 17)), EUNSUPPORTED),
        ("d = 65 / 9 at 33 slots", dict(d=(65, 9), k=31), EUNSUPPORTED)]


@pytest.mark.parametrize("suf", ["f32", "f64"])
@pytest.mark.parametrize("name, changes, want", ROWS, ids=[r[0] for r in ROWS])
def test_status_of_refused_and_empty_calls(name, changes, want, suf):
    args = {n: NUMBERS[n] if n in NUMBERS else (None if n in OPTIONAL else PTR) for n in NAMES}
    args.update({n: v[suf == "f64"] if isinstance(v, tuple) else v for n, v in changes.items()})  # (fp32, fp64) pairs
    assert getattr(_lib.load(), f"mgp_posterior_ns_wave_{suf}")(*[args[n] for n in NAMES]) == want


def test_parameter_list_and_resource_record():
    from muygpys_amd import _abi

    text = open(_abi.HEADER).read()

    def params(name):
        start = text.index(f"int {name}(")
        return " ".join(text[text.index("(", start):text.index(");", start)].split())

    for suf in ("f32", "f64"):
        assert params(f"mgp_posterior_ns_wave_{suf}") == params(f"mgp_posterior_ns_generic_{suf}"), suf
    with open(os.path.join(os.path.dirname(_lib.LIB_PATH), "kernel_resources.json")) as f:
        mine = {n: r for n, r in json.load(f).items() if "ns_wave_forward_kernel" in n}
    assert len(mine) == 13, sorted(mine)
    assert all(r["VGPRs Spill"] == 0 and r["ScratchSize [bytes/lane]"] == 0 for r in mine.values()), mine


def test_mode_switch_and_path_names():
    import torch

    from muygpys_amd import fused

    assert fused.NS_FORWARD_MODES == ("workgroup", "wave") and fused.ns_forward_default() == "workgroup"
    with pytest.raises(ValueError, match="ns_forward"):
        with fused.ns_forward("x"):
            pass
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", "from muygpys_amd import fused"], cwd=root, capture_output=True, text=True,
                       env={**os.environ, "MUYGPYS_HIP_NS_FORWARD": "x"})
    assert r.returncode != 0 and "ValueError" in r.stderr and "MUYGPYS_HIP_NS_FORWARD='x'" in r.stderr, r.stderr[-2000:]
    X, ni = torch.zeros((8, 2)), torch.zeros((4, 3), dtype=torch.int64)
    with pytest.raises(ValueError, match="unknown kernel path"):
        fused.posterior_mean_var(fused.KernelSpec("matern15", "l2", 1.0, 1e-3), X, X, None, ni, torch.zeros(8), path="wave")
