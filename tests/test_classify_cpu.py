"""Classification without a GPU: the numpy oracle against the reference's fixtures (tests/golden/classify, written by
make_golden_classify.py), the properties of those fixtures the GPU tests rely on, the C ABI's argument checks, the
exported names, and -- in the build container, where the reference tree is -- the reference's own functor layer on the
installed hip family: one fused launch and one ``mgp_class_sums_*`` launch per cross-entropy evaluation."""

import ctypes as C
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import classify_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "classify")
NAMES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "*.npz")))
REF = "/root/reference/src"


def load(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    g = {k: z[k] for k in z.files}
    g["meta"] = json.loads(str(g["meta"]))
    return g


def test_the_fixture_set_covers_the_cases():
    metas = [load(n)["meta"] for n in NAMES]
    assert {m["classes"] for m in metas} == {2, 3, 10}
    assert {tuple(m["encoding"]) for m in metas} == {(-1, 1), (0, 1)}
    assert {m["aniso"] for m in metas} == {False, True} and {m["k"] for m in metas} == {12, 30}
    assert all(len(m["probes"]) >= 3 for m in metas)


@pytest.mark.parametrize("name", NAMES)
def test_oracle_reproduces_the_reference_losses(name):
    g = load(name)
    targets = g["labels"][g["batch_indices"]]
    np.testing.assert_allclose(O.cross_entropy(g["mean"], targets), g["cross_entropy"], rtol=1e-8, atol=1e-8)
    np.testing.assert_allclose(O.mse(g["mean"], targets), g["mse"], rtol=1e-8, atol=1e-8)
    sums = O.class_sums(g["mean"], targets)
    assert sums[2] == g["mean"].size and sums[3] == g["mean"].shape[0]
    np.testing.assert_allclose(sums[1] / sums[2], g["mse"], rtol=1e-8)


def test_oracle_clips_like_log_loss():
    """Rows whose softmax leaves [eps, 1 - eps]: logits +-60 on the wrong class give -log(eps) = 36.04 per row in
    fp64, not the unclipped 120; sklearn's log_loss (1.7: clip to the machine epsilon of the probabilities) agrees."""
    from scipy.special import softmax
    from sklearn.metrics import log_loss

    pred = np.array([[60.0, -60.0], [-60.0, 60.0], [0.3, -0.2], [60.0, -60.0]])
    target = np.array([[-1.0, 1.0], [-1.0, 1.0], [1.0, -1.0], [1.0, -1.0]])
    ref = log_loss(np.where(target > 0, 1.0, 0.0), softmax(pred, axis=1), normalize=False)
    got = O.cross_entropy(pred, target)
    np.testing.assert_allclose(got, ref, rtol=1e-12)
    eps = np.finfo(np.float64).eps
    # row 0: the one-hot probability e^-120 is clipped up to eps; rows 1, 3: 1 is clipped down to 1 - eps
    np.testing.assert_allclose(got, -np.log(eps) - 2 * np.log(1 - eps) + np.log1p(np.exp(-0.5)), rtol=1e-12)
    rows = O.cross_entropy_rows(pred, target)
    assert abs(rows[0] - 36.0437) < 1e-3 and rows[0] < 120.0  # (unclipped: 120)
    # three classes, two clipped rows, fp32 epsilon
    pred3 = np.array([[60.0, 0.0, -60.0], [1.0, 2.0, 0.5], [-60.0, 0.0, 60.0]], dtype=np.float32)
    target3 = np.array([[0, 0, 1], [0, 1, 0], [0, 1, 0]], dtype=np.float32)
    ref3 = log_loss(target3, softmax(pred3, axis=1), normalize=False)
    np.testing.assert_allclose(O.cross_entropy(pred3, target3, np.float32), ref3, rtol=1e-6)
    # the cotangent: zero where the one-hot probability is clipped, softmax - one_hot elsewhere
    grad = O.cross_entropy_grad(pred, target)
    assert np.all(grad[[0, 1, 3]] == 0.0)  # (clipped at either end)
    np.testing.assert_allclose(grad[2], softmax(pred, axis=1)[2] - np.array([1.0, 0.0]), rtol=1e-12)


@pytest.mark.parametrize("name", NAMES[:2])
def test_oracle_cotangent_is_the_derivative(name):
    g = load(name)
    mean, targets = g["mean"], g["labels"][g["batch_indices"]]
    grad = O.cross_entropy_grad(mean, targets)
    rng = np.random.default_rng(0)
    for _ in range(5):
        i, c = rng.integers(mean.shape[0]), rng.integers(mean.shape[1])
        h = 1e-6
        hi, lo = mean.copy(), mean.copy()
        hi[i, c] += h
        lo[i, c] -= h
        fd = (O.cross_entropy(hi, targets) - O.cross_entropy(lo, targets)) / (2 * h)
        np.testing.assert_allclose(grad[i, c], fd, rtol=1e-5, atol=1e-8)


@pytest.mark.parametrize("name", NAMES)
def test_oracle_partition_reproduces_classify_any(name):
    g = load(name)
    first, nonconstant, sel, nn_sel = O.partition(g["labels"], g["test_nn_indices"])
    assert np.array_equal(nonconstant, g["nonconstant"])
    assert np.array_equal(g["predictions"][~nonconstant], first[~nonconstant])  # constant rows: exact
    assert np.array_equal(sel, np.where(g["nonconstant"])[0]) and nn_sel.shape == (len(sel), g["meta"]["k"])


@pytest.mark.parametrize("name", NAMES)
def test_fixtures_hold_what_the_generator_asserted(name):
    g = load(name)
    share = g["nonconstant"].mean()
    assert 0.10 < share < 0.90, share  # both branches of the partition are exercised
    assert O.near_ties(g["predictions"], 1e-3).mean() <= 0.01
    assert O.near_ties(g["mean"], 1e-3).mean() <= 0.01
    if "cutoffs" not in g:
        return
    cutv, alpha, beta = g["cutv"], g["alpha"], g["beta"]
    np.testing.assert_allclose(cutv, np.linspace(0.01, 20, 1999), rtol=0, atol=0)
    a2, b2 = O.interval_curves(g["mean"], g["batch_variance"], g["correct_mask"], cutv)
    np.testing.assert_allclose(a2, alpha, atol=1e-12)
    np.testing.assert_allclose(b2, beta, atol=1e-12)
    nc, ni = int(g["correct_mask"].sum()), int((~g["correct_mask"]).sum())
    objectives = [alpha + beta, 2 * alpha + beta, 4 * alpha + beta, 10 * alpha + beta, ni * alpha + nc * beta]
    for obj, cut in zip(objectives, g["cutoffs"]):
        i = int(np.argmin(obj))
        assert cutv[i] == cut and 0 < i < len(cutv) - 1  # an interior grid point ...
        lowest = np.where(obj == obj[i])[0]
        # ... and a strict minimum: one interior plateau, strictly below both ends of the grid
        assert obj[i] < obj[0] and obj[i] < obj[-1] and obj[i] < obj[i - 1]
        assert lowest[-1] - lowest[0] + 1 == len(lowest) and lowest[-1] < len(cutv) - 1
    # make_masks / do_uq of the reference, restated
    m1, v = g["uq_means"][:, 1], g["uq_variances"]
    masks = np.array([(m1 - c * v < 0.0) & (m1 + c * v > 0.0) for c in g["cutoffs"]])
    assert np.array_equal(masks, g["masks"])
    assert np.all(g["uq_variances"][~g["nonconstant"]] == 0.0)


def _lib():
    from muygpys_amd import _lib

    return _lib.load()


def test_new_symbols_are_declared_and_exported():
    from muygpys_amd import _abi, _lib

    lib = _lib.load()
    declared = _lib.exported_names_from_header()
    for base in ("class_sums", "class_partition", "class_scatter"):
        for suf in ("f32", "f64"):
            assert f"mgp_{base}_{suf}" in _abi.signatures()
            assert f"mgp_{base}_{suf}" in declared and hasattr(lib, f"mgp_{base}_{suf}")
    from muygpys_amd._src.optimize.loss import hip as L
    from muygpys_amd.examples import classify
    from muygpys_amd.fused import class_value_and_grad  # noqa: F401
    from muygpys_amd.optimize.loss import cross_entropy_fn  # noqa: F401

    assert callable(L._cross_entropy_fn)
    for name in ("classify_any", "classify_two_class_uq", "make_masks", "do_uq", "train_two_class_interval"):
        assert callable(getattr(classify, name))


def test_class_abi_rejects_bad_arguments_without_a_gpu():
    lib = _lib()
    buf = (C.c_double * 64)()
    idx = (C.c_int64 * 64)()
    p, i = C.cast(buf, C.c_void_p), C.cast(idx, C.c_void_p)
    for sums in (lib.mgp_class_sums_f32, lib.mgp_class_sums_f64):
        es = 4 if sums is lib.mgp_class_sums_f32 else 8

        def call(pred=p, target=p, ts=None, bi=None, b=4, R=3, loss=0, gs=1.0, hd=1.5, grad=None, out=p, scratch=p, fn=sums, es=es):
            return fn(pred, target, R * es if ts is None else ts, bi, b, R, loss, gs, hd, grad, out, scratch, None)

        assert call(R=1) == -2 and call(R=0) == -2 and call(R=63) == -2  # fewer than two labels / beyond the kernels
        assert call(R=-1) == -1 and call(b=-1) == -1
        for bad in (dict(pred=None), dict(target=None), dict(out=None), dict(scratch=None), dict(loss=2), dict(hd=0.0),
                    dict(ts=es), dict(ts=3 * es + 1)):
            assert call(**bad) == -1, bad
    for part in (lib.mgp_class_partition_f32, lib.mgp_class_partition_f64):
        ok = dict(labels=p, n=8, R=2, ni=i, b=4, k=3, pred=p, flags=p, count=i, sel=i, nn_sel=i, scratch=p)
        for bad in (dict(labels=None), dict(ni=None), dict(pred=None), dict(flags=None), dict(count=None), dict(sel=None),
                    dict(nn_sel=None), dict(scratch=None), dict(n=0), dict(R=0), dict(b=-1), dict(k=0)):
            a = dict(ok, **bad)
            assert part(a["labels"], a["n"], a["R"], a["ni"], a["b"], a["k"], a["pred"], a["flags"], a["count"], a["sel"],
                        a["nn_sel"], a["scratch"], None) == -1, bad
    for scat in (lib.mgp_class_scatter_f32, lib.mgp_class_scatter_f64):
        assert scat(None, None, i, 2, 4, 2, p, None, None) == -1
        assert scat(p, None, None, 2, 4, 2, p, None, None) == -1
        assert scat(p, None, i, 2, 4, 2, None, None, None) == -1
        assert scat(p, p, i, 2, 4, 2, p, None, None) == -1      # a variance source without a destination
        assert scat(p, None, i, 5, 4, 2, p, None, None) == -1   # more solved rows than rows
        assert scat(p, None, i, -1, 4, 2, p, None, None) == -1 and scat(p, None, i, 2, 4, 0, p, None, None) == -1
        assert scat(p, None, i, 0, 4, 2, p, None, None) == 0    # nothing to scatter: no launch


def test_new_kernels_spill_nothing():
    from muygpys_amd import build

    build.build()
    res = json.load(open(os.path.join(build.LIBDIR, "kernel_resources.json")))
    mine = {k: v for k, v in res.items() if "3mgp" in k and "class_" in k}
    assert len(mine) >= 9, sorted(mine)  # sums, flags, scatter in two precisions; reduce, scan, compact
    for name, r in mine.items():
        assert r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["ScratchSize [bytes/lane]"] == 0, (name, r)


def test_loss_raises_below_two_labels_before_touching_a_device():
    import torch

    from muygpys_amd._src.optimize.loss import hip as L
    from muygpys_amd import _lib

    real = _lib.require_cuda
    _lib.require_cuda = lambda *a: None
    try:
        for shape in ((5,), (5, 1)):
            with pytest.raises(NotImplementedError, match="two or more labels"):
                L._cross_entropy_fn(torch.zeros(shape), torch.zeros(shape))
    finally:
        _lib.require_cuda = real


FUNCTOR_SCRIPT = r"""
import collections, importlib.metadata as md, sys, types
_v = md.version; md.version = lambda n: "0.9.0" if n == "MuyGPyS" else _v(n)
bo = types.ModuleType("bayes_opt"); bo.BayesianOptimization = object; sys.modules["bayes_opt"] = bo
import numpy as np, torch
import MuyGPyS
import muygpys_amd.integration as hip_backend
hip_backend.install(require_device=False)
# no GPU in the build container: record the C-ABI calls instead of making them
from muygpys_amd import _lib
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
from MuyGPyS.gp.deformation import Isotropy, l2
from MuyGPyS.gp.hyperparameter import FixedScale, Parameter
from MuyGPyS.gp.kernels import Matern
from MuyGPyS.gp.noise import HomoscedasticNoise
from MuyGPyS.optimize import L_BFGS_B_optimize
from MuyGPyS.optimize.loss import cross_entropy_fn
rng = np.random.default_rng(0)
X = torch.from_numpy(rng.normal(size=(200, 6)))
Y = hip_backend.table(torch.from_numpy(np.where(rng.normal(size=(200, 3)) > 0, 1.0, -1.0)))
bi = torch.arange(0, 40); ni = torch.from_numpy(rng.integers(40, 200, size=(40, 8)))
m = MuyGPS(kernel=Matern(smoothness=Parameter(1.5), deformation=Isotropy(l2, length_scale=Parameter(2.0, (0.1, 10.0)))),
           noise=HomoscedasticNoise(1e-3), scale=FixedScale())
cross, pair, y_b, y_nn = m.make_train_tensors(bi, ni, X, Y)
assert type(pair).__name__ == "LazyDiffs" and type(y_nn).__name__ == "LazyTargets", (type(pair), type(y_nn))
obj = L_BFGS_B_optimize.make_obj_fn(m, y_b, y_nn, cross, pair, loss_fn=cross_entropy_fn)
for rep in range(3):
    calls.clear()
    obj(length_scale=1.5)
    fused = sum(v for k, v in calls.items() if k.startswith("posterior"))
    assert fused == 1 and calls["class_sums"] == 1, dict(calls)   # one fused launch, one sums launch
    assert set(calls) <= {k for k in calls if k.startswith("posterior")} | {"class_sums", "table_pack"}, dict(calls)
print("classify-ok")
"""


@pytest.mark.skipif(not os.path.isdir(REF), reason="the reference tree exists only in the build container")
def test_reference_functor_layer_evaluates_cross_entropy_in_two_launches():
    env = dict(os.environ, PYTHONPATH=REF + os.pathsep + ROOT, PYTHONDONTWRITEBYTECODE="1", MUYGPYS_BACKEND="numpy")
    r = subprocess.run([sys.executable, "-c", FUNCTOR_SCRIPT], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "classify-ok" in r.stdout, r.stdout[-1500:] + r.stderr[-3000:]
