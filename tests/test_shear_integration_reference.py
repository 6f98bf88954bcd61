"""The shear family inside the real MuyGPyS package (where the reference is importable; skipped elsewhere, like
tests/test_integration_reference.py).

* CPU, build container: after ``integration.install()`` the reference's ``MuyGPyS.gp.kernels.experimental`` and
  ``MuyGPyS.gp.noise.shear`` import, their backend names resolve to the hip functions, and the reference's OWN
  ShearKernel / ShearKernel2in3out / ShearNoise33 on lazy handles -- its ``diffs[..., None, :]`` shape rule included --
  end in ONE mgp_shear_posterior launch per mean + variance (recorded: no GPU there).
* GPU (h): a real ShearKernel / ShearNoise33 and ShearKernel2in3out / HomoscedasticNoise model on the hip backend, in a
  fresh process, against the same model on the reference's numpy backend in another."""

import os
import subprocess
import sys

import numpy as np
import pytest

REF = "/root/reference/src"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
needs_reference = pytest.mark.skipif(not os.path.isdir(REF), reason="the reference tree exists only in the build container")

SHIMS = r"""
import importlib.metadata as md, sys, types
_v = md.version; md.version = lambda n: "0.9.0" if n == "MuyGPyS" else _v(n)
bo = types.ModuleType("bayes_opt"); bo.BayesianOptimization = object; sys.modules["bayes_opt"] = bo
"""

INSTALL_SCRIPT = SHIMS + r"""
import inspect
import MuyGPyS
import muygpys_amd.integration as hip_backend
hip_backend.install(require_device=False)
import MuyGPyS.gp.kernels.experimental as E
import MuyGPyS.gp.noise.shear as NS
import MuyGPyS._src.gp.kernels.shear as KS
import MuyGPyS._src.gp.noise as N
HIP = "muygpys_amd._src.gp.kernels.shear.hip"
for n in ("_shear_33_fn", "_shear_Kin23_fn", "_shear_Kcross23_fn"):
    assert getattr(KS, n).__module__ == HIP, (n, getattr(KS, n).__module__)
assert N._shear_perturb33.__module__ == "muygpys_amd._src.gp.noise.hip"
assert inspect.signature(E.ShearKernel.__init__).parameters["_backend_fn"].default.__module__ == HIP
p = inspect.signature(E.ShearKernel2in3out.__init__).parameters
for n in ("_backend_Kin_fn", "_backend_Kcross_fn", "_backend_Kout_fn"):
    assert p[n].default.__module__ == HIP, n
assert inspect.signature(NS.ShearNoise33.__init__).parameters["_backend_fn"].default is N._shear_perturb33
print("shear-installed")
"""

LAZY_SCRIPT = SHIMS + r"""
import collections
import numpy as np, torch
import MuyGPyS
import muygpys_amd.integration as hip_backend
hip_backend.install(require_device=False)
from muygpys_amd import _lib, lazy
import muygpys_amd._src.math.hip as mmh
calls = collections.Counter()
def fake_fn(base, dtype):
    def call(*args):
        calls[base] += 1
        return 0
    return call
_lib.fn = fake_fn
_lib.require_cuda = lambda *a: None
_lib.stream_ptr = lambda: None
mmh._device = lambda: torch.device("cpu")
from MuyGPyS.gp import MuyGPS
from MuyGPyS.gp.deformation import DifferenceIsotropy, F2
from MuyGPyS.gp.hyperparameter import FixedScale, Parameter
from MuyGPyS.gp.kernels.experimental import ShearKernel, ShearKernel2in3out
from MuyGPyS.gp.noise import HomoscedasticNoise
from MuyGPyS.gp.noise.shear import ShearNoise33
rng = np.random.default_rng(0)
X = torch.from_numpy(rng.uniform(size=(200, 2)))
Y = torch.from_numpy(rng.normal(size=(200, 3)))
for b, k in ((40, 8), (8, 8)):  # b == k: the reference's shape rule does not fire, the handle's kind decides
    bi = torch.arange(b)
    ni = torch.from_numpy(rng.integers(40, 200, size=(b, k)))
    for kind in ("33", "23"):
        dfm = DifferenceIsotropy(F2, length_scale=Parameter(0.3))
        if kind == "33":
            m = MuyGPS(kernel=ShearKernel(deformation=dfm), noise=ShearNoise33(1e-3), scale=FixedScale())
            tab = Y
        else:
            m = MuyGPS(kernel=ShearKernel2in3out(deformation=dfm), noise=HomoscedasticNoise(1e-3), scale=FixedScale())
            tab = Y[:, 1:].contiguous()
        cross, pair, y_nn = m.make_predict_tensors(bi, ni, X[:b], X, tab)
        assert type(pair).__name__ == "LazyDiffs" and type(cross).__name__ == "LazyDiffs", (type(pair), type(cross))
        calls.clear()
        Kin, Kc = m.kernel(pair), m.kernel(cross)
        assert isinstance(Kin, lazy.LazyShearCov) and Kin.kind == "pairwise" and Kin.model == kind
        assert isinstance(Kc, lazy.LazyShearCov) and Kc.kind == "crosswise" and Kc.model == kind
        assert Kc.diffs.unit_axis == (b != k)  # the reference's diffs[..., None, :] stayed a handle
        assert not calls, dict(calls)           # building the covariances launches nothing
        m.posterior_mean(Kin, Kc, y_nn.swapaxes(-2, -1))
        m.posterior_variance(Kin, Kc)
        assert calls["shear_posterior"] == 1 and set(calls) == {"shear_posterior"}, dict(calls)
print("shear-lazy-ok")
"""

CASE = r"""
import numpy as np
rng = np.random.default_rng(3)
N, b, k, ell, eps = 300, 12, 20, 0.05, 1e-3
Xh, Yh = rng.uniform(size=(N, 2)), rng.normal(size=(N, 3))
bih = np.arange(b)
nih = np.stack([rng.choice(np.arange(b, N), size=k, replace=False) for _ in range(b)])
"""

RUN = r"""
from MuyGPyS.gp import MuyGPS
from MuyGPyS.gp.deformation import DifferenceIsotropy, F2
from MuyGPyS.gp.hyperparameter import FixedScale, Parameter
from MuyGPyS.gp.kernels.experimental import ShearKernel, ShearKernel2in3out
from MuyGPyS.gp.noise import HomoscedasticNoise
from MuyGPyS.gp.noise.shear import ShearNoise33
out = {}
for kind in ("33", "23"):
    dfm = DifferenceIsotropy(F2, length_scale=Parameter(ell))
    if kind == "33":
        m = MuyGPS(kernel=ShearKernel(deformation=dfm), noise=ShearNoise33(eps), scale=FixedScale())
    else:
        m = MuyGPS(kernel=ShearKernel2in3out(deformation=dfm), noise=HomoscedasticNoise(eps), scale=FixedScale())
    cross, pair, y_nn = m.make_predict_tensors(bi, ni, X[:b], X, Y)
    y_nn = y_nn.swapaxes(-2, -1)
    if kind == "23":
        y_nn = y_nn[:, 1:, :]
    Kin, Kc = m.kernel(pair), m.kernel(cross)
    out["mean" + kind] = host(m.posterior_mean(Kin, Kc, y_nn))
    out["var" + kind] = host(m.posterior_variance(Kin, Kc))
np.savez(sys.argv[1], **out)
print("ran")
"""

NUMPY_SCRIPT = SHIMS + CASE + r"""
import MuyGPyS
X, Y, bi, ni = Xh, Yh, bih, nih
host = np.asarray
""" + RUN

HIP_SCRIPT = SHIMS + CASE + r"""
import torch
import MuyGPyS
import muygpys_amd.integration as hip_backend
hip_backend.install()
from muygpys_amd import _lib
X = torch.tensor(Xh, device="cuda", dtype=torch.float64)
Y = torch.tensor(Yh, device="cuda", dtype=torch.float64)
bi, ni = torch.tensor(bih, device="cuda"), torch.tensor(nih, device="cuda")
host = lambda t: t.double().cpu().numpy()
""" + RUN + r"""
assert "shear_posterior_kernel" in _lib.last_kernel(), _lib.last_kernel()
"""


def _run(script, *args, backend="numpy", timeout=300):
    env = dict(os.environ, PYTHONPATH=REF + os.pathsep + ROOT, PYTHONDONTWRITEBYTECODE="1", MUYGPYS_BACKEND=backend)
    return subprocess.run([sys.executable, "-c", script, *args], env=env, capture_output=True, text=True,
                          timeout=timeout)


@needs_reference
def test_shear_family_installs_into_reference_package():
    r = _run(INSTALL_SCRIPT)
    assert r.returncode == 0 and "shear-installed" in r.stdout, r.stderr[-2000:]


@needs_reference
def test_reference_shear_functors_reach_one_fused_launch():
    r = _run(LAZY_SCRIPT)
    assert r.returncode == 0 and "shear-lazy-ok" in r.stdout, r.stdout[-1500:] + r.stderr[-3000:]


@pytest.mark.gpu
@needs_reference
def test_h_reference_shear_model_on_hip_matches_numpy_backend(tmp_path):
    ref, hip = str(tmp_path / "numpy.npz"), str(tmp_path / "hip.npz")
    r = _run(NUMPY_SCRIPT, ref)
    assert r.returncode == 0 and "ran" in r.stdout, r.stderr[-3000:]
    r = _run(HIP_SCRIPT, hip)
    assert r.returncode == 0 and "ran" in r.stdout, r.stderr[-3000:]
    a, b = np.load(ref), np.load(hip)
    for key in a.files:
        want, got = a[key], b[key]
        assert got.shape == want.shape, (key, got.shape, want.shape)
        atol = 1e-5 * np.sqrt(np.mean(want**2))
        assert np.all(np.abs(got - want) <= 1e-5 * np.abs(want) + atol), (key, float(np.abs(got - want).max()))
