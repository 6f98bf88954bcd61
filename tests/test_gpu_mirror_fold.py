"""GPU: the mirror-folded elimination (csrc/mgp_fused_wave_kernel.h, phase 4F: lane l of a quarter-wave owns rows l
and 31 - l of a 32-slot neighbourhood) and the pipelined Gram loop in front of it, against the fp64 oracle.

Shapes: the built-in (30, 40) and (29, 40), and run-time compiled folded shapes at the fold's edges -- k = 16 (the
first folded nn_count: the query row is row 16, the last lane's long row), k = 17, k = 30 with d = 8 (two 16-byte
groups per row: the Gram pipeline is all prologue).  Batches of 1 (one task, no partner), 2, 3 (odd tail), 5 and 4 099.

A launch's grid is the device's resident capacity, so a batch of 4 099 gives every workgroup at most one task and no
elimination ever sees a pair.  The cases therefore run twice: in this process at the default grid, and in ONE child
process with MUYGPYS_HIP_JIT=force (the policy is read once per process: even one-neighbourhood calls take the
specialised kernels there) and one resident workgroup per CU, where 2 050 tasks are some eight per workgroup -- pairs,
and an unpaired last task wherever a workgroup's count is odd.  In-process, a batch of 24 581 forms pairs too."""

import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from oracle import muygps_oracle as orc
from tests.util import RTOL, assert_close, to_dev

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

BATCHES = (1, 2, 3, 5, 4099)
B = 4099
N = 3000
SHARD = 1000
INPROC_SHAPES = ((30, 40), (29, 40))                     # (k, d), one response
CHILD_SHAPES = ((30, 40), (29, 40), (16, 8), (17, 8), (30, 8))
PACKED_SHAPES = ((30, 40), (16, 8))
BROKEN = np.arange(3, B, 149)                            # non-SPD neighbourhoods: both halves of a task, every pair position
CLUSTER_TASKS = np.arange(5, B // 2, 37)                 # tasks (two neighbourhoods each) that trip the Gram guard


def _ell(d):
    return float(np.sqrt(2 * d))


def _problem(k, d):
    """Tables and one master batch of B neighbourhoods (float32-representable values); shorter batches are its heads."""
    rng = np.random.default_rng(100 * k + d)
    X = rng.normal(size=(N, d)).astype(np.float32).astype(np.float64)
    y = (np.sin(X[:, : min(d, 3)].sum(1)) + 0.05 * rng.normal(size=N)).astype(np.float32).astype(np.float64)
    bi = rng.integers(0, N, size=B)
    ni = np.stack([rng.choice(N - 1, size=k, replace=False) for _ in range(B)])
    ni = ni + (ni >= bi[:, None])
    return X, y, bi, ni


def _cluster_problem(k, d):
    """`cluster1e-2` of tests/test_gpu_gram_stress.py: a tight cluster of neighbours three length scales from the query
    (its pairs trip the Gram form's cancellation guard), for the tasks CLUSTER_TASKS of a batch whose other
    neighbourhoods are the benign ones of _problem().  -> X, Q, y, bi, ni of the mixed batch."""
    X0, y0, bi0, ni0 = _problem(k, d)
    rng = np.random.default_rng(7 * k + d)
    ell = _ell(d)
    nbs = np.concatenate([2 * CLUSTER_TASKS, 2 * CLUSTER_TASKS + 1])
    nc = nbs.size
    Qc = rng.normal(size=(nc, d))
    C = rng.normal(size=(nc, d))
    C *= (3 * ell / np.linalg.norm(C, axis=1))[:, None]
    Xc = (Qc[:, None, :] + C[:, None, :] + 1e-2 * ell * rng.normal(size=(nc, k, d)) / np.sqrt(d)).reshape(nc * k, d)
    Xc, Qc = Xc.astype(np.float32).astype(np.float64), Qc.astype(np.float32).astype(np.float64)
    X = np.concatenate([X0, Xc])
    Q = np.concatenate([X0, Qc])
    y = np.concatenate([y0, np.sin(Xc[:, : min(d, 3)].sum(1)).astype(np.float32).astype(np.float64)])
    bi, ni = bi0.copy(), ni0.copy()
    bi[nbs] = N + np.arange(nc)
    ni[nbs] = N + np.arange(nc * k).reshape(nc, k)
    return X, Q, y, bi, ni


def compute_cases(k, d, packed_too):
    """Every launch of one shape -> {name: array}.  Runs in this process and in the child."""
    from muygpys_amd import _lib
    from muygpys_amd.fused import KernelSpec, posterior_mean_var

    out = {}
    X, y, bi, ni = _problem(k, d)
    Xd, yd = to_dev(X, torch.float32), to_dev(y, torch.float32)

    def run(bi_, ni_, nugget=1e-3, packed=False, Q=None, Xt=None, yt=None):
        info = torch.zeros(1, dtype=torch.int32, device="cuda")
        res = posterior_mean_var(KernelSpec("matern15", "l2", _ell(d), nugget), Xd if Q is None else Q, Xd if Xt is None else Xt,
                                 to_dev(bi_), to_dev(ni_), yd if yt is None else yt, want_ykinvy=True, info=info, packed=packed)
        torch.cuda.synchronize()
        return np.stack([r.cpu().numpy().reshape(-1) for r in res]), int(info.item())

    for b in BATCHES:
        out[f"b{b}"], bad = run(bi[:b], ni[:b])
        out[f"b{b}_info"] = np.array(bad)
    out["served"] = np.array(_lib.last_kernel())
    out["shards"] = np.concatenate([run(bi[s:s + SHARD], ni[s:s + SHARD])[0] for s in range(0, B, SHARD)], axis=1)
    if packed_too:
        out["packed"] = run(bi, ni, packed=True)[0]
        out["packed_served"] = np.array(_lib.last_kernel())
    # non-SPD: a duplicated neighbour and no nugget, in neighbourhoods spread over every position of a pair -- the first
    # two rows (short rows of the first two lanes), or the first and the last (a short row and a long row).  The copy
    # of ROW 0 is what makes the count exact in fp32: the first pivot is exactly 1, so the first step leaves the
    # copy's row exactly zero and its pivot is 0, not a rounding error of either sign
    for tag, (c0, c1) in (("lo", (1, 0)), ("hi", (k - 1, 0))):
        nb = ni.copy()
        nb[BROKEN, c0] = nb[BROKEN, c1]
        out[f"spd_{tag}"], bad = run(bi, nb, nugget=0.0)
        out[f"spd_{tag}_info"] = np.array(bad)
    out["spd_clean"] = run(bi, ni, nugget=0.0)[0]
    mates = np.unique(np.concatenate([BROKEN[:6] - 1, BROKEN[:6] + 1]))
    out["spd_mates"] = mates
    out["spd_alone"] = np.concatenate([run(bi[m:m + 1], ni[m:m + 1], nugget=0.0)[0] for m in mates], axis=1)
    # Gram guard: guarded tasks among benign ones
    Xc, Qc, yc, bic, nic = _cluster_problem(k, d)
    Xcd, Qcd, ycd = to_dev(Xc, torch.float32), to_dev(Qc, torch.float32), to_dev(yc, torch.float32)
    out["guard"], bad = run(bic, nic, Q=Qcd, Xt=Xcd, yt=ycd)
    out["guard_info"] = np.array(bad)
    out["guard_benign"] = run(bi, ni, Q=Qcd, Xt=Xcd, yt=ycd)[0]
    return out


def _key(k, d):
    return f"k{k}d{d}"


@pytest.fixture(scope="module")
def inproc():
    return {_key(k, d): compute_cases(k, d, (k, d) in PACKED_SHAPES) for k, d in INPROC_SHAPES}


CHILD = r"""
import sys
sys.path.insert(0, %(root)r)
import numpy as np
from muygpys_amd import _lib
import tests.test_gpu_mirror_fold as m
assert _lib.load().mgp_jit_mode() == 2
res = {}
for k, d in m.CHILD_SHAPES:
    for name, v in m.compute_cases(k, d, (k, d) in m.PACKED_SHAPES).items():
        res[m._key(k, d) + "/" + name] = v
np.savez(%(out)r, **res)
"""


@pytest.fixture(scope="module")
def child():
    """The same launches with every static shape served by its specialised kernel and one workgroup per CU."""
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "cases.npz")
        env = dict(os.environ, MUYGPYS_HIP_JIT="force", MGP_WAVE_PER_CU="1", MGP_JIT_PER_CU="1", PYTHONDONTWRITEBYTECODE="1")
        r = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT, "out": path}], env=env, capture_output=True,
                           text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        z = np.load(path)
        res = {}
        for name in z.files:
            shape, case = name.split("/", 1)
            res.setdefault(shape, {})[case] = z[name]
    return res


_ORACLE = {}


def _oracle(k, d, kind):
    """fp64 reference of the master batch (computed once per shape)."""
    if (k, d, kind) not in _ORACLE:
        if kind == "benign":
            X, y, bi, ni = _problem(k, d)
            Q = X
        else:
            X, Q, y, bi, ni = _cluster_problem(k, d)
        m, v = orc.posterior_mean_var(orc.Spec("matern15", "l2", _ell(d), 1e-3), Q, X, bi, ni, y)
        _ORACLE[(k, d, kind)] = (np.asarray(m).reshape(-1), np.asarray(v).reshape(-1))
    return _ORACLE[(k, d, kind)]


def _cases(request, where, k, d):
    return request.getfixturevalue(where)[_key(k, d)]


WHERE = [("inproc", s) for s in INPROC_SHAPES] + [("child", s) for s in CHILD_SHAPES]
IDS = [f"{w}-k{s[0]}-d{s[1]}" for w, s in WHERE]


def _one_kernel_for_every_batch(where, shape):
    """Whether launches of 1 and of 4 099 neighbourhoods are served by the same instantiation, so that their bits can be
    compared: always in the child, and in this process for the built-in shape.  Any other static shape is served by
    the run-time-shape kernel below 4 096 neighbourhoods and, from there on, by its specialised kernel IF an earlier
    test of the session happened to load it -- another summation order."""
    return where == "child" or shape == (30, 40)


SAME = [(w, s) for w, s in WHERE if _one_kernel_for_every_batch(w, s)]
SAME_IDS = [i for i, (w, s) in zip(IDS, WHERE) if _one_kernel_for_every_batch(w, s)]


@pytest.mark.parametrize("where,shape", WHERE, ids=IDS)
def test_every_batch_size_matches_the_oracle(request, where, shape):
    k, d = shape
    c = _cases(request, where, k, d)
    m_ref, v_ref = _oracle(k, d, "benign")
    if where == "child":  # every shape there is a static one: the folded kernel
        assert f",{k},1,{d}," in str(c["served"]).replace(" ", ""), c["served"]
    for b in BATCHES:
        assert int(c[f"b{b}_info"]) == 0
        got = c[f"b{b}"]
        print(f"{where} k={k} d={d} b={b}: max |mean err| {np.abs(got[0] - m_ref[:b]).max():.3e}, max |var err| {np.abs(got[1] - v_ref[:b]).max():.3e}")
        assert_close(got[0], m_ref[:b], RTOL["float32"], f"mean (b={b})")
        assert_close(got[1], v_ref[:b], RTOL["float32"], f"var (b={b})")
        assert np.isfinite(got[2]).all()


@pytest.mark.parametrize("where,shape", SAME, ids=SAME_IDS)
def test_shards_concatenate_bit_for_bit(request, where, shape):
    """A neighbourhood's outputs do not depend on its wave-mates or its place in a pair: shards of 1 000 put every
    neighbourhood behind the first shard into another workgroup and pair position."""
    c = _cases(request, where, *shape)
    assert np.array_equal(c["b4099"], c["shards"])
    for b in BATCHES[:-1]:
        assert np.array_equal(c[f"b{b}"], c["b4099"][:, :b])


@pytest.mark.parametrize("where,shape", [w for w in WHERE if w[1] in PACKED_SHAPES],
                         ids=[i for i, w in zip(IDS, WHERE) if w[1] in PACKED_SHAPES])
def test_prepared_and_plain_tables_agree_bit_for_bit(request, where, shape):
    c = _cases(request, where, *shape)
    if where == "child":
        assert f",{shape[0]},1,{shape[1]},true,false,true,true>" in str(c["packed_served"]).replace(" ", ""), c["packed_served"]
    assert np.array_equal(c["packed"], c["b4099"])


@pytest.mark.parametrize("where,shape", WHERE, ids=IDS)
def test_non_spd_neighbourhoods_are_counted_and_leave_their_partners_alone(request, where, shape):
    c = _cases(request, where, *shape)
    healthy = np.setdiff1d(np.arange(B), BROKEN)
    for tag in ("lo", "hi"):
        got = c[f"spd_{tag}"]
        assert int(c[f"spd_{tag}_info"]) == BROKEN.size, tag
        assert np.isnan(got[:2, BROKEN]).all(), tag
        assert np.isfinite(got[:, healthy]).all(), tag
        # the others -- wave-mates and pair partners of the broken ones among them -- as in the batch without a broken
        # one, and as when run alone
        assert np.array_equal(got[:, healthy], c["spd_clean"][:, healthy]), tag
        if _one_kernel_for_every_batch(where, shape):
            assert np.array_equal(got[:, c["spd_mates"]], c["spd_alone"]), tag


@pytest.mark.parametrize("where,shape", WHERE, ids=IDS)
def test_gram_guard_of_a_task_paired_with_benign_tasks(request, where, shape):
    """Tasks whose distances are recomputed in the difference form (phase 2G) among tasks that are not: both are right,
    and the benign ones return the bits they return in a batch without a guarded task."""
    k, d = shape
    c = _cases(request, where, k, d)
    m_ref, v_ref = _oracle(k, d, "cluster")
    assert int(c["guard_info"]) == 0
    assert_close(c["guard"][0], m_ref, RTOL["float32"], "mean")
    assert_close(c["guard"][1], v_ref, RTOL["float32"], "var")
    guarded = np.concatenate([2 * CLUSTER_TASKS, 2 * CLUSTER_TASKS + 1])
    benign = np.setdiff1d(np.arange(B), guarded)
    assert np.array_equal(c["guard"][:, benign], c["guard_benign"][:, benign])


def test_a_batch_beyond_the_grid_pairs_tasks_in_process():
    """24 581 neighbourhoods are more tasks than the default grid has workgroups: pairs, unpaired last tasks and an odd
    neighbourhood tail at the built-in shape, shards bit for bit and a sample against the oracle."""
    from muygpys_amd.fused import KernelSpec, posterior_mean_var

    k, d, b = 30, 40, 24581
    X, y, _, _ = _problem(k, d)
    rng = np.random.default_rng(99)
    bi = rng.integers(0, N, size=b)
    ni = rng.integers(0, N - 1, size=(b, k))
    ni = ni + (ni >= bi[:, None])
    Xd, yd, bid, nid = to_dev(X, torch.float32), to_dev(y, torch.float32), to_dev(bi), to_dev(ni)
    spec = KernelSpec("matern15", "l2", _ell(d), 1e-3)
    whole = posterior_mean_var(spec, Xd, Xd, bid, nid, yd, want_ykinvy=True)
    parts = [posterior_mean_var(spec, Xd, Xd, bid[s:s + 7001], nid[s:s + 7001], yd, want_ykinvy=True) for s in range(0, b, 7001)]
    torch.cuda.synchronize()
    for i, w in enumerate(whole):
        assert torch.equal(w, torch.cat([p[i] for p in parts]))
    pick = np.unique(np.concatenate([np.arange(40), np.arange(b - 40, b), rng.integers(0, b, size=300)]))
    m_ref, v_ref = orc.posterior_mean_var(orc.Spec("matern15", "l2", _ell(d), 1e-3), X, X, bi[pick], ni[pick], y)
    assert_close(whole[0].cpu().numpy()[pick], np.asarray(m_ref).reshape(-1), RTOL["float32"], "mean")
    assert_close(whole[1].cpu().numpy()[pick], v_ref, RTOL["float32"], "var")
