"""The fused backward (csrc/mgp_capi.hip: posterior_backward) behind its three kernel rungs -- F, the backward
instantiation of the forward wave kernel (csrc/mgp_backward_dlt.hip); W, backward_wave_kernel
(csrc/mgp_backward_wave_kernel.h); L, the LDS workgroup kernel backward_kernel (csrc/mgp_backward.hip): the problem
recipe, a per-neighbourhood reference in plain dense algebra that runs in a chosen number format, the launch rules
restated in Python, and the case list with the kernel name each case must be served by.

CPU only (numpy; torch is not imported here).  tests/backward_rung_runner.py runs the cases of one rung on the GPU
in a process of its own, tests/test_gpu_backward_rungs.py compares what it stored with the reference below, and
tests/test_backward_cases_cpu.py asserts without a GPU that the reference is right, that the restated rules are the
library's, that the sample covers what it claims and that its inputs can tell a wrong kernel from a right one.

The recipe is that of tests/posterior_cases.py: a neighbour table uniform on [0, 1]^d (n = 300), a separate uniform
query table (nq = 53), responses sin(3 sum(x) / sqrt(d) + r) + 0.1 normal, neighbourhoods of k distinct random rows,
b = 37, the isotropic length scale sqrt(d / 6), the anisotropic one that times (1 + 0.3 U) per feature, a noise table
0.05 (1 + 3 U) per table row, scalar noise 0.05, batch noise table[nn_idx]; rbf with F2, matern05 with l2 or F2, the
other three with l2.  One deliberate difference: ``batch_idx`` is drawn WITH replacement, so neighbourhoods share
query rows (and, the table being small, neighbour rows) and the atomic accumulation is exercised.  On one shared
table a neighbourhood never holds its own batch row unless the case says so (``zero``): a pair at zero distance is
a case of its own.  The upstream cotangents are standard normal."""

import functools
from types import SimpleNamespace

import numpy as np

from tests.posterior_cases import CNAME, KERNELS, NO_M05

SEED = 20261021
N, NQ, B = 300, 53, 37
LONG_B = 20011  # the second pass of every persistent loop
NOISE = 0.05
BAD_ROWS = (0, 18, 36)  # the neighbourhoods of the non-SPD cases
# tests/util.py, DESIGN section 2: 1e-5 in fp64, three times the forward band in fp32
RTOL = {"float64": 1e-5, "float32": 3 * 1e-3}
ES = {"float32": 4, "float64": 8}
EUNSUPPORTED = -2
# cases whose first draw missed a condition of tests/test_backward_cases_cpu.py: {case id: draw}
RESEED = {}
# muygpys_amd/build.py: PREWARM_BWD, the shapes whose backward instantiation build() compiles, (element size, k, d)
PREWARM_BWD = ((8, 40, 8), (8, 40, 16), (8, 50, 16), (8, 32, 8), (4, 30, 16), (4, 20, 40), (4, 25, 8), (8, 30, 40), (4, 50, 8),
               (4, 40, 16), (4, 10, 8), (4, 30, 100))
BUILTIN_BWD = ((4, 30, 40), (8, 50, 8))
# compiled on demand by the runner (mgp_jit_prepare_backward); a case of these may skip where that call fails.  The
# smallest k of F, the long cases' k = 5 and the first dealt-triangle shape: 2 to 3 s of compiler each.  (The far ends --
# 64 slots, rows of 100 features -- are among the prepared shapes: fp64 (62, 64) compiles for five minutes, fp32
# (30, 128) for one.)
ON_DEMAND_BWD = ((4, 3, 4), (4, 5, 4), (8, 5, 2), (8, 31, 2))


# ---- the launch rules, restated ----------------------------------------------------------------------------------------
CU_LDS_BYTES = 160 * 1024


def lds_row_stride(es, k):
    """csrc/mgp_lds_factor.h: a row of k + 1 entries in an odd number of 16-byte slots."""
    E = 16 // es
    return (((k + 1 + E - 1) // E) | 1) * E


def backward_lds_bytes(es, k, dc):
    """csrc/mgp_backward.hip: [idx][S (k+2) SP][Q (k+1) SP][X (k+1)(dc + E)][il dc][lacc dc][colb 64][piv k][red 2][flag]."""
    SP = lds_row_stride(es, k)
    n = ((k + 2) & ~1) * 8
    n += ((k + 2) * SP + (k + 1) * SP + (k + 1) * (dc + 16 // es) + 2 * dc + 64 + k + 2) * es + 16
    return (n + 15) & ~15


def feature_chunk(d, lds_bytes):
    """csrc/mgp_launch.h: (dc, bytes, fits): a multiple of 8, at most 64, shrunk until it fits, at least 8."""
    dc = (d + 7) // 8 * 8 if d < 64 else 64
    while dc > 8 and lds_bytes(dc) > CU_LDS_BYTES:
        dc -= 8
    return dc, lds_bytes(dc), lds_bytes(dc) <= CU_LDS_BYTES


def lds_rule(es, k, d):
    """(threads, dc, chunks) of backward_kernel at a shape, None where the system does not fit."""
    dc, _, fits = feature_chunk(d, lambda c: backward_lds_bytes(es, k, c))
    if not fits:
        return None
    threads = 64 if k + 2 <= 64 else (128 if k + 2 <= 128 else 256)
    return threads, dc, -(-d // dc)


def max_nn_count_backward(es):
    k = 1
    while backward_lds_bytes(es, k + 1, 8) <= CU_LDS_BYTES:
        k += 1
    return k


def wave_rule(es, k, d, feat, ls_count):
    """(NP, DG, KFIX, HYPER) of backward_wave_kernel at a shape (csrc/mgp_backward_wave.hip, launch_bwd_dg,
    launch_bwd_np), None where it declines.  ``feat``: a feature cotangent is asked for."""
    E = 16 // es
    rows = k + 2
    if d > 16 * E or rows > 64:
        return None
    NP = 32 if rows <= 32 else 64
    dv = -(-d // E)
    kfix = 0
    if es == 8:
        if NP == 64:
            if d > 8:
                return None
            dg = 4
        elif dv <= 4:
            dg = 4
        elif dv <= 8:
            dg = 8
        else:
            return None
    elif dv <= 4:
        dg = 4
    elif dv <= 8:
        dg = 8
    elif dv <= 10:
        dg = 10
        if NP == 32 and k == 30 and dv == 10:
            kfix = 30
    elif dv <= 12:
        dg = 12
    else:
        dg = 16
    return NP, dg, kfix, (not feat) and ls_count > 1


def _row_slots(es, k, d):
    E = 16 // es
    CH, DCAP = 2 * E, (128 if es == 4 else 64)
    if k < 3 or d < E or d % E != 0 or -(-d // CH) * CH > DCAP:
        return 0
    if k + 2 <= 32:
        return 32
    return 64 if es == 4 and k + 2 <= 64 else 0


def _dlt_shape(k, d):
    return 33 <= k + 2 <= 64 and d >= 2 and d % 2 == 0 and (d + 3) // 4 * 4 <= 64


def fwd_rule(es, k, d, feat, kernel, aligned):
    """(NP, gram, built_in, dealt) of the forward kernel's backward instantiation (csrc/mgp_backward_dlt.hip:
    launch_backward_fwd) where its code, once compiled, serves the call; None where it declines."""
    if not aligned:
        return None
    gram = es == 4 and kernel != "matern05"  # wave_gram(..., bwd): the fp64 backward is in the difference form
    builtin = (k == 50 and d == 8) if es == 8 else (k == 30 and d == 40 and gram)
    if es == 8:
        if feat and _row_slots(8, k, d) == 0:
            return None
        if builtin:
            return 64, gram, True, True
        if _dlt_shape(k, d):
            return 64, gram, False, True
    elif builtin:
        return 32, gram, True, False
    NP = _row_slots(es, k, d)
    return (NP, gram, False, False) if NP else None


def served(c):
    """(kernel name, neighbourhoods per task) that the case's rung environment must serve it with: F = no switch,
    W = MGP_BACKWARD_DLT=0, L = MGP_BACKWARD_LDS=1; (None, 0): MGP_EUNSUPPORTED, no launch."""
    es, k, d = ES[c["dtype"]], c["k"], c["d"]
    t = CNAME[c["dtype"]]
    feat = c["want"] in ("all", "nn")
    ls_count = d if c["aniso"] else 1
    tf = ("false", "true")
    if c["rung"] == "F":
        f = fwd_rule(es, k, d, feat, c["kernel"], not c["off"])
        if f is not None:
            NP, gram, builtin, _ = f
            return (f"mgp::fused_wave_kernel<{t},{NP},{k},1,{d},true,false,false,{tf[gram]},false,backward>"
                    + ("" if builtin else " [run-time compiled]")), 64 // NP
    if c["rung"] in ("F", "W"):
        w = wave_rule(es, k, d, feat, ls_count)
        if w is not None:
            NP, dg, kfix, hyper = w
            return f"mgp::backward_wave_kernel<{t},{NP},{dg},{kfix},{tf[hyper]}>", 64 // NP
    r = lds_rule(es, k, d)
    if r is None:
        return None, 0
    return f"mgp::backward_kernel<{t}> [threads={r[0]},dc={r[1]}]", 1


# ---- the case list -----------------------------------------------------------------------------------------------------
def _metric(kernel, j):
    return "F2" if kernel == "rbf" else (("l2", "F2")[j % 2] if kernel == "matern05" else "l2")


class _Deck:
    """Kernels round-robin over the five (over those a rung serves), with the metric of the pairing."""

    def __init__(self):
        self.j = 0

    def draw(self, kernels=KERNELS):
        self.j += 1
        kernel = kernels[self.j % len(kernels)]
        return kernel, _metric(kernel, self.j // len(kernels))


def _case(deck, rung, dtype, k, d, tag, *, R=1, b=B, aniso=False, noise="scalar", bi=True, own_query=False, want="all", gm=True,
          gv=True, loocv=None, off=False, zero=None, bad=False, kernel=None, metric=None):
    """``want``: all (both feature cotangents -- one buffer on a shared table --, responses, length scale, noise) |
    hyper (length scale and noise) | hyper+tg | nn (grad_feat_nn alone).  ``loocv``: None | all | yk (the LOOCV entry
    with three cotangents / with grad_ykinvy alone, the other two zero: the entry refuses a NULL one).  ``zero``: None | self (the batch row among its own neighbours) | dup
    (one neighbour listed twice).  ``bad``: the non-SPD case."""
    # the Gram form of fp32 F is another compiled shape than the difference form Matern-1/2 takes: build() prepares the
    # former, so F in fp32 draws from the other four
    kernels = NO_M05 if (rung == "F" and dtype == "float32") else KERNELS
    drawn = deck.draw(kernels)
    kernel, metric = (kernel, metric or _metric(kernel, 0)) if kernel else drawn
    if zero == "self":  # (under l2, where the direction of a zero difference is undefined)
        kernel, metric = ("matern25" if kernel == "rbf" else kernel), "l2"
    if loocv:
        assert R == 1 and not own_query and want == "hyper"
    if bad:
        noise = "batch"
    c = dict(rung=rung, dtype=dtype, k=k, d=d, R=R, b=b, kernel=kernel, metric=metric, aniso=aniso, noise=noise, bi=bi,
             own_query=own_query, want=want, gm=gm, gv=gv, loocv=loocv, off=off, zero=zero, bad=bad, tag=tag)
    c["id"] = (f"{rung}-{dtype}-k{k}-d{d}-R{R}-b{b}-{kernel}-{metric}-{'aniso' if aniso else 'iso'}-{noise}-{'bi' if bi else 'nobi'}"
               f"-{'q' if own_query else 'same'}-{want}-{'m' if gm else ''}{'v' if gv else ''}{'-loocv_' + loocv if loocv else ''}"
               f"{'-off' if off else ''}{'-zero_' + zero if zero else ''}{'-bad' if bad else ''}-{tag}")
    c["expect"], c["per_task"] = served(c)
    return c


def _modes(deck, rung, dtype, shapes, feat_ok=(True, True), long_d=4):
    """The argument modes on the two ``shapes`` of a rung and type in turn.  ``feat_ok``: whether the rung's kernel has
    feature cotangents at each shape (the dealt triangle has none: its cases ask for hyper+tg, and one request for
    feature cotangents there must name another kernel)."""
    out = []
    j = [0]

    def add(tag, **kw):
        i = j[0] % 2
        j[0] += 1
        k, d = shapes[i]
        if not feat_ok[i] and kw.get("want", "all") in ("all", "nn"):
            if kw.get("own_query") or kw.get("want") == "nn" or kw.get("off") or kw.get("zero") == "self":
                i = 1 - i
                k, d = shapes[i]
                assert feat_ok[i]
            else:
                kw["want"] = "hyper+tg"
        out.append(_case(deck, rung, dtype, k, d, tag, **kw))

    add("noise-scalar", noise="scalar")
    add("noise-table", noise="table", aniso=True)
    add("noise-batch", noise="batch")
    add("noise-batch2", noise="batch", aniso=True)
    add("nobi", bi=False, own_query=True, noise="table")
    add("nobi2", bi=False, aniso=True)
    add("query", own_query=True, aniso=True, noise="batch")
    add("query2", own_query=True)
    add("shared", own_query=False, aniso=True)
    add("R2", R=2, noise="table")
    add("R5", R=5, aniso=True, own_query=True)
    add("R5b", R=5, noise="batch")
    add("nomean", gm=False, aniso=True)
    add("novar", gv=False, R=2)
    add("nomean2", gm=False, own_query=True, noise="table")
    add("novar2", gv=False, aniso=True, noise="batch")
    add("nn-only", want="nn", aniso=True)
    add("nn-only2", want="nn", own_query=True)
    add("hyper", want="hyper", aniso=True, noise="table")
    add("hyper-iso", want="hyper")
    add("loocv", want="hyper", loocv="all", aniso=True, noise="table")
    add("loocv2", want="hyper", loocv="all")
    add("loocv-yk", want="hyper", loocv="yk", aniso=True)
    add("loocv-yk2", want="hyper", loocv="yk", noise="batch")
    add("off", off=True, own_query=True, aniso=True)
    add("off2", off=True)
    add("b1", b=1, own_query=True, noise="batch")
    add("b1s", b=1, aniso=True)
    add("b2", b=2, aniso=True, noise="table")
    add("b2q", b=2, own_query=True)
    add("zero-self", zero="self", kernel=None if (rung == "F" and dtype == "float32") else "matern05", metric="l2")
    add("zero-self2", zero="self", aniso=True, noise="table")
    # (on one shared table the two ends of a zero-distance pair are one row and whatever the pair contributes cancels
    # in the sum: grad_feat_nn alone leaves the neighbour's end standing)
    add("zero-self-nn", zero="self", want="nn", kernel=None if (rung == "F" and dtype == "float32") else "matern05", metric="l2")
    add("zero-dup", zero="dup", aniso=True)
    add("zero-dup2", zero="dup", own_query=True, noise="batch")
    add("bad", bad=True, aniso=True, own_query=True)
    add("bad2", bad=True)
    # the second pass of the persistent loop: k = 5 in a small-d shape that stays in the rung
    out.append(_case(deck, rung, dtype, 5, long_d, "long", b=LONG_B, aniso=True, noise="batch", bi=False, own_query=True))
    return out


def _cases():
    cases = []
    deck = _Deck()
    # ---- W: backward_wave_kernel, MGP_BACKWARD_DLT=0 ------------------------------------------------------------------
    w32 = [(1, 1), (2, 3), (30, 16), (29, 17), (30, 32), (13, 33), (30, 40), (30, 37), (29, 40), (20, 41), (30, 48), (12, 49), (30, 64),
           # 64 slots ((40, 24): DG 8, the one instantiation that the shapes above leave out)
           (31, 4), (62, 16), (40, 24), (45, 40), (33, 47), (62, 64)]
    w64 = [(30, 2), (7, 1), (30, 8), (30, 9), (3, 15), (30, 16), (31, 8), (50, 6), (62, 1), (62, 8), (31, 9), (40, 16)]
    for dtype, shapes in (("float32", w32), ("float64", w64)):
        for i, (k, d) in enumerate(shapes):
            # every (T, NP, DG, KFIX) twice: all outputs, and anisotropic with grad_ls and grad_noise alone (HYPER)
            cases.append(_case(deck, "W", dtype, k, d, "shape", aniso=bool(i % 2), noise=("scalar", "table", "batch")[i % 3],
                               own_query=bool(i % 3 == 1), R=(1, 2, 5)[i % 3]))
            cases.append(_case(deck, "W", dtype, k, d, "shape-hyper", aniso=True, want="hyper", noise=("batch", "scalar", "table")[i % 3]))
    cases += _modes(deck, "W", "float32", ((30, 40), (45, 38)))
    cases += _modes(deck, "W", "float64", ((30, 8), (50, 6)), long_d=2)
    # ---- L: backward_kernel, MGP_BACKWARD_LDS=1 -----------------------------------------------------------------------
    lds = [("float32", 1, 3), ("float64", 1, 2), ("float32", 62, 5), ("float64", 62, 4), ("float32", 63, 6), ("float64", 63, 3),
           ("float32", 126, 4), ("float32", 127, 4), ("float32", 137, 8), ("float64", 96, 6), ("float32", 137, 1), ("float64", 96, 1),
           ("float32", 137, 70), ("float64", 90, 70), ("float64", 96, 69)]
    lds += [(dtype, 20, d) for d in (1, 7, 8, 9, 64, 65, 70) for dtype in ("float32", "float64")]
    for i, (dtype, k, d) in enumerate(lds):
        cases.append(_case(deck, "L", dtype, k, d, "shape", aniso=bool(i % 2), noise=("scalar", "table", "batch")[i % 3],
                           own_query=bool(i % 3 == 1), R=(1, 2, 5)[i % 3] if k < 90 else 1))
    # one past the limit: MGP_EUNSUPPORTED, no launch
    cases.append(_case(deck, "L", "float32", 138, 8, "past-limit"))
    cases.append(_case(deck, "L", "float64", 97, 8, "past-limit"))
    cases += _modes(deck, "L", "float32", ((70, 20), (20, 70)))
    cases += _modes(deck, "L", "float64", ((66, 9), (21, 65)))
    # ---- F: the forward kernel's backward instantiation ---------------------------------------------------------------
    for es, k, d in BUILTIN_BWD + PREWARM_BWD + ON_DEMAND_BWD:
        if k == 5:  # (the long cases' shapes: in _modes)
            continue
        dtype = "float32" if es == 4 else "float64"
        dealt = fwd_rule(es, k, d, False, "matern15", True)[3]
        i = len(cases)
        # the dealt-triangle shapes run with hyper-parameter outputs only
        cases.append(_case(deck, "F", dtype, k, d, "shape", aniso=bool(i % 2), noise=("scalar", "table", "batch")[i % 3],
                           own_query=bool(i % 3 == 1) and not dealt, R=(1, 2, 5)[i % 3], want="hyper+tg" if dealt else "all"))
        cases.append(_case(deck, "F", dtype, k, d, "shape-hyper", aniso=True, want="hyper", noise=("batch", "scalar", "table")[i % 3]))
        if dealt:  # a request for feature cotangents there must name W or L
            cases.append(_case(deck, "F", dtype, k, d, "shape-feat", aniso=bool(i % 2)))
    cases += _modes(deck, "F", "float32", ((30, 40), (50, 8)))
    cases += _modes(deck, "F", "float64", ((50, 8), (30, 40)), feat_ok=(False, True), long_d=2)
    ids = [c["id"] for c in cases]
    assert len(set(ids)) == len(ids), sorted(i for i in ids if ids.count(i) > 1)
    return cases


CASES = _cases()
BY_ID = {c["id"]: c for c in CASES}
RUNGS = ("F", "W", "L")


def rung_cases(rung):
    return [c for c in CASES if c["rung"] == rung]


def prepared_shape(c):
    """The (element size, k, d) whose compiled code an F case needs: 'builtin' | 'prewarm' | 'demand' | None (the case
    names W or L)."""
    if c["rung"] != "F" or "fused_wave_kernel" not in (c["expect"] or ""):
        return None
    key = (ES[c["dtype"]], c["k"], c["d"])
    if "run-time compiled" not in c["expect"]:
        return "builtin"
    assert key in PREWARM_BWD + ON_DEMAND_BWD, key
    return "prewarm" if key in PREWARM_BWD else "demand"


# ---- the problem of a case ---------------------------------------------------------------------------------------------
def _build(c, draw):
    rng = np.random.default_rng([SEED, sum(map(ord, c["id"])), len(c["id"]), draw])
    k, R, d, b = c["k"], c["R"], c["d"], c["b"]
    Xn = rng.uniform(size=(N, d))
    Y = np.stack([np.sin(3.0 * Xn.sum(1) / np.sqrt(d) + r) + 0.1 * rng.normal(size=N) for r in range(R)], axis=1)
    nq = max(NQ, b)  # (no batch index: neighbourhood i reads query row i)
    Xq = rng.uniform(size=(nq, d)) if c["own_query"] else Xn
    bi = rng.integers(0, NQ if c["own_query"] else N, size=b) if c["bi"] else np.arange(b)  # WITH replacement
    shared = not c["own_query"]
    assert not shared or b <= N
    if shared:  # k of the n - 1 other rows
        ni = np.argsort(rng.uniform(size=(b, N - 1)), axis=1)[:, :k]
        ni = ni + (ni >= bi[:, None])
    else:
        ni = np.argsort(rng.uniform(size=(b, N)), axis=1)[:, :k]
    if c["zero"] == "self":
        assert shared
        ni[np.arange(b), np.arange(b) % k] = bi
    elif c["zero"] == "dup":
        assert k >= 2
        ni[:, k - 1] = ni[:, 0]
    iso = float(np.sqrt(d / 6.0))
    ls = iso * (1.0 + 0.3 * rng.uniform(size=d)) if c["aniso"] else iso
    table = NOISE * (1.0 + 3.0 * rng.uniform(size=N))
    noise_rows = np.full((b, k), NOISE) if c["noise"] == "scalar" else table[ni]
    gm = rng.normal(size=(b, R)) if c["gm"] else None
    gv = rng.normal(size=b) if c["gv"] else None
    gy = rng.normal(size=b) if c["loocv"] else None
    if c["loocv"] == "yk":  # (the LOOCV entry takes all three pointers: the other two cotangents are zero)
        gm, gv = np.zeros((b, R)), np.zeros(b)
    for a in (Xn, Y, Xq, ni, bi, table, noise_rows, gm, gv, gy):
        if a is not None:
            a.setflags(write=False)
    return SimpleNamespace(Xn=Xn, Y=Y, Xq=Xq, ni=ni, bi=bi, ls=ls, table=table, noise_rows=noise_rows, gm=gm, gv=gv, gy=gy, b=b,
                           kernel=c["kernel"], metric=c["metric"])


@functools.lru_cache(maxsize=None)
def problem(case_id):
    """The inputs of a case (read-only, shared): Xn (n, d), Y (n, R), Xq (the query table, Xn itself unless the case
    has its own), ni (b, k), bi (b,) (arange(b) where the call passes no batch index), ls (a float or (d,)), the noise
    table (n,), the noise diagonal of every neighbourhood (b, k) whatever the layout it arrives in, and the cotangents
    gm (b, R) / gv (b,) / gy (b,) (None: the call passes NULL)."""
    return _build(BY_ID[case_id], RESEED.get(case_id, 0))


def bad_noise_rows(c, P):
    """The noise diagonal of the non-SPD case: -2.0 at the first, the middle and the last neighbour of neighbourhoods 0,
    18 and 36 (a strictly negative pivot, no rounding-dependent zero)."""
    assert c["bad"] and c["noise"] == "batch" and P.b == B
    noise = np.array(P.noise_rows)
    noise[list(BAD_ROWS), [0, c["k"] // 2, c["k"] - 1]] = -2.0
    return noise


# ---- the reference: one neighbourhood at a time, plain dense algebra, in a chosen number format -------------------------
def _kernel_and_derivative(kernel, x, T):
    """(kappa(x), kappa'(x)) of oracle.muygps_oracle.KERNELS / KERNEL_DERIVS, every constant in the format of ``x``."""
    if kernel == "rbf":
        e = np.exp(-x / T(2))
        return e, -e / T(2)
    if kernel == "matern05":
        e = np.exp(-x)
        return e, -e
    if kernel == "matern15":
        s = x * T(np.sqrt(3.0))
        e = np.exp(-s)
        return (T(1) + s) * e, -T(3) * x * e
    if kernel == "matern25":
        s = x * T(np.sqrt(5.0))
        e = np.exp(-s)
        return (T(1) + s + s * s / T(3)) * e, -(T(5) / T(3)) * x * (T(1) + s) * e
    assert kernel == "maternInf", kernel
    e = np.exp(-(x * x) / T(2))
    return e, -x * e


def vjp_rows(P, dtype=np.float64, rows=None, *, noise_rows=None, bi=None, Xq=None, subgradient=0.0):
    """The vector-Jacobian product of every neighbourhood in ``rows`` (default: all) by itself, in ``dtype``:

        L_i = gm_i . mean_i + gv_i var_i + gy_i y^T K^-1 y,   mean = c^T K^-1 Y,  var = 1 - c^T K^-1 c,

    as dense algebra on the (k + 1) x (k + 1) covariance of the neighbours and the query row: two solves, the
    cotangent matrix G = dL/dK_ij = gv a a^T - a w^T - gy u u^T (a = K^-1 c, w = K^-1 Y gm, u = K^-1 y; the K-bar of
    include/muygpys_hip.h with w = gm u), dL/dc = w - 2 gv a, then the chain through kappa and the metric to the
    pairwise differences.  Returns grad_ls (m, ls_count), grad_noise (m, k) and the neighbourhood's own contributions
    g_q (m, d) to its query row, g_nn (m, k, d) to its neighbours' rows and g_tg (m, k, R) to their responses.
    A pair at zero distance under l2 contributes ``subgradient`` times the direction (1, ..., 1) / sqrt(d): 0 is
    torch.norm's subgradient; anything else is a mutant.  ``noise_rows`` / ``bi`` / ``Xq``: other inputs than the
    problem's (mutants, the non-SPD case)."""
    T = np.dtype(dtype).type
    rows = np.arange(P.b) if rows is None else np.asarray(rows)
    bi = P.bi if bi is None else bi
    Xn, Xq = P.Xn.astype(dtype), (P.Xq if Xq is None else Xq).astype(dtype)
    Yt = P.Y.astype(dtype)
    nz = (P.noise_rows if noise_rows is None else noise_rows).astype(dtype)
    k, d, R = P.ni.shape[1], Xn.shape[1], Yt.shape[1]
    aniso, l2 = np.ndim(P.ls) == 1, P.metric == "l2"
    il = (T(1) / np.asarray(P.ls, dtype=dtype)) if aniso else np.ones(d, dtype=dtype)
    ell = None if aniso else T(P.ls)
    lp = None if aniso else (ell if l2 else ell * ell)  # x = r / l | r / l^2
    m = len(rows)
    out = SimpleNamespace(grad_ls=np.empty((m, d if aniso else 1), dtype=dtype), grad_noise=np.empty((m, k), dtype=dtype),
                          g_q=np.empty((m, d), dtype=dtype), g_nn=np.empty((m, k, d), dtype=dtype), g_tg=np.empty((m, k, R), dtype=dtype),
                          rows=rows)
    gm_all = np.zeros((P.b, R), dtype=dtype) if P.gm is None else P.gm.astype(dtype)
    gv_all = np.zeros(P.b, dtype=dtype) if P.gv is None else P.gv.astype(dtype)
    gy_all = np.zeros(P.b, dtype=dtype) if P.gy is None else P.gy.astype(dtype)
    step = max(1, 3_000_000 // ((k + 1) * (k + 1) * d))
    eye = np.eye(k, dtype=bool)
    for s in range(0, m, step):
        r = rows[s:s + step]
        n_ = len(r)
        Z = np.concatenate([Xn[P.ni[r]], Xq[bi[r]][:, None, :]], axis=1)  # (m, k + 1, d): the neighbours, then the query row
        D = Z[:, :, None, :] - Z[:, None, :, :]
        S = D * il
        F2 = np.sum(S * S, axis=-1)
        rad = np.sqrt(F2) if l2 else F2
        x = rad if aniso else rad / lp
        Kf, kp = _kernel_and_derivative(P.kernel, x, T)
        K = Kf[:, :k, :k].copy()
        K[:, eye] += nz[r]
        c = Kf[:, :k, k]
        Yn = Yt[P.ni[r]]  # (m, k, R)
        A = np.linalg.solve(K, np.concatenate([c[:, :, None], Yn], axis=2))
        assert A.dtype == np.dtype(dtype)
        a, U = A[:, :, 0], A[:, :, 1:]
        gm, gv, gy = gm_all[r], gv_all[r], gy_all[r]
        w = np.einsum("bkr,br->bk", U, gm)
        u = U[:, :, 0]  # (the LOOCV term: one response)
        GK = gv[:, None, None] * a[:, :, None] * a[:, None, :] - a[:, :, None] * w[:, None, :] - gy[:, None, None] * u[:, :, None] * u[:, None, :]
        out.grad_noise[s:s + n_] = GK[:, eye]
        out.g_tg[s:s + n_] = a[:, :, None] * gm[:, None, :]
        if P.gy is not None:
            out.g_tg[s:s + n_, :, 0] += T(2) * gy[:, None] * u
        G = np.zeros((n_, k + 1, k + 1), dtype=dtype)
        G[:, :k, :k] = GK
        G[:, np.eye(k + 1, dtype=bool)] = T(0)   # (the diagonal of the covariance is kappa(0): constant)
        G[:, :k, k] = w - T(2) * gv[:, None] * a  # dL/dc, once per ordered pair
        gx = G * kp                              # dL/dx
        if aniso:
            grad = gx
        else:
            out.grad_ls[s:s + n_, 0] = np.sum(gx * (-(T(1) if l2 else T(2)) * x / ell), axis=(1, 2))
            grad = gx / lp                       # dL/d rad
        if l2:
            pos = rad > 0
            unit = np.where(pos[..., None], S / np.where(pos, rad, T(1))[..., None], T(subgradient) / T(np.sqrt(d)))
            gS = grad[..., None] * unit
            gS[:, np.eye(k + 1, dtype=bool)] = T(0)
        else:
            gS = T(2) * grad[..., None] * S
        if aniso:
            out.grad_ls[s:s + n_] = np.sum(gS * (-D * il * il), axis=(1, 2))
        gD = gS * il
        gZ = gD.sum(axis=2) - gD.sum(axis=1)
        out.g_nn[s:s + n_] = gZ[:, :k]
        out.g_q[s:s + n_] = gZ[:, k]
    return out


def accumulate(c, P, v, bi=None):
    """What the launch adds to its three accumulated buffers from the per-neighbourhood contributions ``v``:
    {"gq": (nq, d) | None, "gnn": (n, d) | None, "gtg": (n, R) | None}.  On one shared table (the case has no query
    table of its own) with both feature cotangents the two are ONE buffer, returned as "gnn"."""
    bi = P.bi if bi is None else bi
    r = v.rows
    out = dict(gq=None, gnn=None, gtg=None)
    if c["want"] in ("all", "nn"):
        out["gnn"] = np.zeros(P.Xn.shape, dtype=np.float64)
        np.add.at(out["gnn"], P.ni[r], v.g_nn.astype(np.float64))
    if c["want"] == "all":
        if c["own_query"]:
            out["gq"] = np.zeros(P.Xq.shape, dtype=np.float64)
            np.add.at(out["gq"], bi[r], v.g_q.astype(np.float64))
        else:
            np.add.at(out["gnn"], bi[r], v.g_q.astype(np.float64))
    if c["want"] in ("all", "hyper+tg") and P.gm is not None:
        out["gtg"] = np.zeros(P.Y.shape, dtype=np.float64)
        np.add.at(out["gtg"], P.ni[r], v.g_tg.astype(np.float64))
    elif c["want"] in ("all", "hyper+tg"):
        out["gtg"] = np.zeros(P.Y.shape, dtype=np.float64)  # (no mean cotangent: the buffer is passed and stays as it was)
    return out


def compared(c, P, v, bi=None):
    """Every output the GPU test compares, as {name: array}: grad_ls and grad_noise per neighbourhood, unsummed, and the
    accumulated tables that the case asks for."""
    out = {"gls": v.grad_ls, "gnz": v.grad_noise}
    out.update({name: a for name, a in accumulate(c, P, v, bi).items() if a is not None})
    return out


def band_error(got, ref):
    """The smallest t with |got - ref| <= t |ref| + t rms(ref) (tests/util.assert_close); where the reference is all
    zero (a buffer the call must leave as it was): 0 for an exact match, inf otherwise."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    rms = float(np.sqrt(np.mean(ref**2)))
    if rms == 0.0:
        return 0.0 if np.array_equal(got, ref) else float("inf")
    return float(np.max(np.abs(got - ref) / (np.abs(ref) + rms)))


@functools.lru_cache(maxsize=None)
def reference(case_id):
    """The fp64 reference of a case: (per-neighbourhood pieces, the compared outputs); for a non-SPD case over the
    other 34 neighbourhoods.  Computed once, shared among the tests."""
    c, P = BY_ID[case_id], problem(case_id)
    rows = np.setdiff1d(np.arange(P.b), BAD_ROWS) if c["bad"] else None
    v = vjp_rows(P, np.float64, rows)
    return v, compared(c, P, v)
