"""The argument modes of the fused posterior (csrc/mgp_capi.hip: posterior) for every kernel family behind the
dispatcher: the problem recipe, the family table, the seeded factor sample and a plain restatement of the oracle in a
chosen number format.

CPU only (numpy; torch is not imported here).  Every family carries its own copy of the code that reads the three noise
layouts, ``batch_idx == NULL``, a query table of its own, gathered responses and the non-SPD flag;
tests/test_gpu_posterior_modes.py runs the sample below on the GPU and tests/test_posterior_cases_cpu.py asserts, with
the oracle alone, that the sample covers what it claims and that its inputs can tell a wrong mode from a right one.

The recipe: a neighbour table uniform on [0, 1]^d (n = 300), a separate uniform query table (nq = 53), responses
sin(3 sum(x) / sqrt(d) + r) + 0.1 normal, neighbourhoods of k distinct random rows, b = 37, the isotropic length scale
sqrt(d / 6) (covariances O(0.5) at every d), the anisotropic one that times (1 + 0.3 U) per feature, a noise table
0.05 (1 + 3 U) per table row, scalar noise 0.05, batch noise table[nn_idx].  Kernel and metric are paired as in
tests/test_gpu_large.py: rbf with F2, matern05 with l2 or F2, the other three with l2."""

import functools
from types import SimpleNamespace

import numpy as np

SEED = 20261019
N, NQ, B = 300, 53, 37
LONG_B = 20011  # the second pass of every persistent loop, below the run-time-compile threshold (65536)
NOISE = 0.05
KERNELS = ("rbf", "matern05", "matern15", "matern25", "maternInf")
NO_M05 = ("rbf", "matern15", "matern25", "maternInf")
CNAME = {"float32": "float", "float64": "double"}
BAD_ROWS = (0, 18, 36)  # the neighbourhoods of the non-SPD test
# cases whose first draw missed a condition of tests/test_posterior_cases_cpu.py: {case id: draw}
RESEED = {}


# ---- the family table --------------------------------------------------------------------------------------------------
def _shape(k, R, d, path="auto", yk=None, off=False, kernels=None, gathered=None):
    """One shape of an entry.  ``path``: the argument of posterior_mean_var; ``yk`` / ``gathered``: True / False where
    the entry needs it so, None where the sample is free (gathered responses go through the dispatcher, so a named
    path forces the table form); ``off``: the tables start one element off the 16-byte grid; ``kernels``: the kernels
    with which this shape reaches the entry's kernel."""
    if path != "auto":
        assert not gathered
        gathered = False
    return dict(k=k, R=R, d=d, path=path, yk=yk, off=off, kernels=kernels, gathered=gathered)


def _entry(name, family, dtype, prefix, shapes, packed=False, exact=False, kernels=None):
    for s in shapes:
        if s["kernels"] is None:
            s["kernels"] = kernels
    return dict(name=name, family=family, dtype=dtype, prefix=prefix, shapes=shapes, packed=packed, exact=exact)


def _entries():
    out = []
    S = _shape
    for dtype in ("float32", "float64"):
        t, f32 = CNAME[dtype], dtype == "float32"
        wave, fam = f"mgp::fused_wave_kernel<{t},", lambda f: f"{f}/{dtype}"
        odd = 6 if f32 else 5     # a row that the prepared table pads to the next 16-byte group
        unvec = 6 if f32 else 7   # a row that is no whole number of 16-byte groups
        small = 4 if f32 else 2
        rp = 4 if f32 else 2      # responses that ride in the 16-byte slot of a prepared row
        # the run-time-shape wave kernels: <T,NP,0,0,0,piped,coeff,packed,gram>
        out.append(_entry("W32p", fam("wave"), dtype, wave + "32,0,0,0,true,false,false,",
                          [S(30, 1, 8), S(20, 3, 12), S(5, 2, small), S(27, 4, 64), S(12, 1, 16)]))
        out.append(_entry("W32r", fam("wave"), dtype, wave + "32,0,0,0,false,false,false,",
                          [S(20, 3, 3), S(25, 1, 70), S(30, 1, 8, off=True), S(10, 2, 5), S(14, 16, 1)]))
        out.append(_entry("W64p", fam("wave"), dtype, wave + "64,0,0,0,true,false,false,",
                          [S(62, 1, 8), S(47, 16, 16), S(32, 1, small), S(40, 3, 64), S(31, 1, 12)]))
        out.append(_entry("W64r", fam("wave"), dtype, wave + "64,0,0,0,false,false,false,",
                          [S(62, 1, unvec), S(47, 16, 72), S(35, 2, unvec), S(50, 3, 72), S(40, 1, 16, off=True)]))
        out.append(_entry("W32pk", fam("wave"), dtype, wave + "32,0,0,0,true,false,true,",
                          [S(30, 1, 8), S(20, rp - 1, 12), S(20, rp, odd), S(10, 16, odd, gathered=True), S(25, 2, 64)], packed=True))
        out.append(_entry("W64pk", fam("wave"), dtype, wave + "64,0,0,0,true,false,true,",
                          [S(62, 1, 8), S(47, 16, 16, gathered=True), S(40, rp, odd), S(33, 2, 24), S(50, 3, 64, gathered=True)],
                          packed=True))
        # the two built-in static shapes
        for nm, (np_, k, d) in (("S30", (32, 30, 40)), ("S50", (64, 50, 8))):
            for pk in (False, True):
                out.append(_entry(nm + ("pk" if pk else ""), fam("static"), dtype,
                                  wave + f"{np_},{k},1,{d},true,false,{'true' if pk else 'false'},", [S(k, 1, d)], packed=pk))
        # fused_rhs_kernel<T,RC,back,gram[,w3|,fold]>
        rhs = f"mgp::fused_rhs_kernel<{t},"
        if f32:
            out.append(_entry("RHS4g", fam("rhs"), dtype, rhs + "4,false,true>", [
                S(20, 3, 8, "rhs"), S(64, 3, 8), S(33, 1, 40, "rhs"), S(62, 4, 64), S(7, 2, 12, "rhs")], exact=True, kernels=NO_M05))
            out.append(_entry("RHS4d", fam("rhs"), dtype, rhs + "4,false,false>", [
                S(20, 3, 3, "rhs"), S(30, 1, 70, "rhs"), S(25, 2, 8, "rhs", kernels=("matern05",)), S(64, 3, 6), S(63, 4, 70)], exact=True))
            out.append(_entry("RHS16f", fam("rhs"), dtype, rhs + "16,false,", [
                S(60, 16, 8, yk=True), S(20, 5, 3, "rhs", yk=True), S(33, 9, 70, "rhs", yk=True), S(64, 16, 40, yk=True),
                S(12, 7, 12, "rhs", yk=True)]))
            out.append(_entry("RHS16fold", fam("rhs"), dtype, rhs + "16,true,true,fold>", [
                S(64, 16, 44, yk=False), S(20, 5, 48, "rhs", yk=False), S(50, 16, 48, yk=False), S(33, 8, 44, "rhs", yk=False)],
                exact=True, kernels=NO_M05))
            out.append(_entry("RHS16w3", fam("rhs"), dtype, rhs + "16,true,true,w3>", [
                S(64, 5, 64, yk=False, off=True), S(20, 16, 8, "rhs", yk=False, off=True), S(60, 16, 40, yk=False, off=True),
                S(33, 7, 12, "rhs", yk=False, off=True)], exact=True, kernels=NO_M05))
            out.append(_entry("RHS16b", fam("rhs"), dtype, rhs + "16,true,false>", [
                S(64, 16, 6, yk=False), S(20, 5, 70, "rhs", yk=False), S(40, 9, 8, "rhs", yk=False, kernels=("matern05",)),
                S(60, 16, 70, yk=False), S(25, 12, 3, "rhs", yk=False)], exact=True))
            mf = [S(64, 5, 64, yk=False), S(20, 16, 8, "rhs", yk=False), S(60, 16, 40, yk=False), S(33, 7, 12, "rhs", yk=False),
                  S(64, 16, 8, yk=False)]
            out.append(_entry("MF", fam("rhs_mf"), dtype, "mgp::fused_rhs_mf_kernel<16>", mf, exact=True, kernels=NO_M05))
            mfpk = [S(64, 5, 64, yk=False, gathered=False), S(20, 16, 8, yk=False, gathered=False),
                    S(60, 16, 40, yk=False, gathered=False), S(33, 7, 12, yk=False, gathered=False), S(40, 9, 6, yk=False, gathered=False)]
            out.append(_entry("MFpk", fam("rhs_mf"), dtype, "mgp::fused_rhs_mf_kernel<16> [prepared tables]", mfpk, packed=True,
                              exact=True, kernels=NO_M05))
        else:
            out.append(_entry("RHS4", fam("rhs"), dtype, rhs + "4,false,false>", [
                S(20, 3, 8, "rhs"), S(64, 3, 8), S(33, 1, 70, "rhs"), S(62, 4, 64), S(7, 2, 3, "rhs")], exact=True))
            out.append(_entry("RHS16b", fam("rhs"), dtype, rhs + "16,true,false>", [
                S(64, 16, 8, yk=False), S(20, 5, 70, "rhs", yk=False), S(60, 16, 40, yk=False), S(25, 12, 3, "rhs", yk=False)],
                exact=True))
            out.append(_entry("RHS16f", fam("rhs"), dtype, rhs + "16,false,false>", [
                S(60, 16, 8, yk=True), S(20, 5, 3, "rhs", yk=True), S(33, 9, 70, "rhs", yk=True), S(64, 16, 40, yk=True)], exact=True))
        # two waves (fp32) / four waves (fp64) per neighbourhood: 65 .. 128 rows
        wide, wname = (("mgp::fused_wide_kernel<", "wide"), ("mgp::fused_wide64_kernel<", "wide64"))[0 if f32 else 1]
        first = 17 if f32 else 18
        out.append(_entry(f"{wname.upper()}_{first}", fam(wname), dtype, f"{wide}{first}>",
                          [S(65, 1, 3), S(65, 1, 64), S(65, 2, 8), S(65, 1, 20)], exact=True))                      # rows 67, 68
        out.append(_entry(f"{wname.upper()}_24", fam(wname), dtype, f"{wide}24>",
                          [S(89, 3, 3), S(89, 3, 64), S(91, 1, 8), S(80, 15, 40)], exact=True))                     # rows 93, 96
        out.append(_entry(f"{wname.upper()}_32", fam(wname), dtype, f"{wide}32>",
                          [S(111, 16, 3), S(111, 16, 64), S(120, 1, 8), S(120, 1, 3), S(126, 1, 40), S(110, 10, 12)], exact=True))
        # the LDS workgroup kernel: by name, and where the dispatcher ends with it (two feature stages, 17 responses)
        out.append(_entry("GEN", fam("generic"), dtype, f"mgp::fused_generic_kernel<{t}>",
                          [S(12, 3, 3, "generic"), S(70, 1, 70), S(70, 17, 8), S(30, 2, 40, "generic"), S(65, 3, 72)], exact=True))
    return out


ENTRIES = _entries()
FAMILIES = sorted({e["family"] for e in ENTRIES})
# the long case of a family: (entry, k, R, d), the family's smallest shape that gathered responses reach.  fused_rhs_mf
# serves five responses or more, so its gathered tensor has five columns where the others have at most three.
LONG = {"wave": ("W32p", 5, 2, 4), "static": ("S30", 30, 1, 40), "rhs": (None, 62, 2, 8), "rhs_mf": ("MF", 64, 5, 8),
        "wide": ("WIDE_17", 65, 1, 4), "wide64": ("WIDE64_18", 65, 1, 4), "generic": ("GEN", 70, 1, 70)}


def _fix(c, s):
    """The draw of a case, bent to what its shape can reach."""
    if s["kernels"] is not None and c["kernel"] not in s["kernels"]:
        c["kernel"] = s["kernels"][c["j"] % len(s["kernels"])]
    if c["kernel"] == "rbf":
        c["metric"] = "F2"
    elif c["kernel"] != "matern05":
        c["metric"] = "l2"
    if s["gathered"] is not None:
        c["gathered"] = s["gathered"]
    if s["yk"] is not None:
        c["yk"] = s["yk"]
    return c


def _case_id(c):
    return (f"{c['entry']}-{c['dtype']}-k{c['k']}-R{c['R']}-d{c['d']}{'off' if c['off'] else ''}-{c['path']}-{c['kernel']}-{c['metric']}"
            f"-{'aniso' if c['aniso'] else 'iso'}-{c['noise']}-{'gathered' if c['gathered'] else 'table'}-{'bi' if c['bi'] else 'nobi'}"
            f"-{'q' if c['own_query'] else 'same'}-{'yk' if c['yk'] else 'noyk'}-b{c['b']}")


def _cases():
    """The sample: per family one ``spread`` (tests/test_gpu_large.py::_edge_cases) of every factor over the family's
    case slots -- five per entry of one shape, six otherwise, the shapes in turn -- and two cases at b in {1, 2, 3}
    with batch noise, gathered responses and no batch index."""
    cases = []
    for fi, family in enumerate(FAMILIES):
        slots = [(e, e["shapes"][j % len(e["shapes"])], j) for e in ENTRIES if e["family"] == family
                 for j in range(5 if len(e["shapes"]) == 1 else 6)]
        n_cases = len(slots)
        # (what a shape cannot reach is bent by _fix, which may take a value out again: the first draw that keeps all)
        for draw in range(64):
            rng = np.random.default_rng([SEED, fi, draw])

            def spread(values):
                reps = -(-n_cases // len(values))
                return [values[i] for i in rng.permutation(np.tile(np.arange(len(values)), reps)[:n_cases])]

            cols = dict(kernel=spread(list(KERNELS)), metric=spread(["l2", "F2"]), aniso=spread([False, True]),
                        noise=spread(["scalar", "table", "batch"]), gathered=spread([False, True]), bi=spread([True, False]),
                        own_query=spread([False, True]), yk=spread([False, True]))
            drawn = []
            for i, (e, s, j) in enumerate(slots):
                c = dict(entry=e["name"], family=family, dtype=e["dtype"], packed=e["packed"], prefix=e["prefix"], exact=e["exact"],
                         k=s["k"], R=s["R"], d=s["d"], path=s["path"], off=s["off"], b=B, j=j)
                c.update({name: vals[i] for name, vals in cols.items()})
                drawn.append(_fix(c, s))
            served = NO_M05 if family.startswith("rhs_mf") else KERNELS
            if all({c[name] for c in drawn} == set(vals) for name, vals in cols.items() if name not in ("kernel", "yk")) \
                    and {c["kernel"] for c in drawn} == set(served):
                break
        else:
            raise AssertionError(f"{family}: no draw covers every factor value")
        cases += drawn
        # b in {1, 2, 3}: the first two entries of the family that gathered responses reach, in their first such shape
        reach = [(e, s) for e in ENTRIES if e["family"] == family for s in e["shapes"][:1] if s["gathered"] is not False]
        reach += [(e, s) for e in ENTRIES if e["family"] == family for s in e["shapes"][1:] if s["gathered"] is not False]
        for j, (b, (e, s)) in enumerate(zip(((1, 2), (2, 3), (1, 3))[fi % 3], reach)):
            c = dict(entry=e["name"], family=family, dtype=e["dtype"], packed=e["packed"], prefix=e["prefix"], exact=e["exact"],
                     k=s["k"], R=s["R"], d=s["d"], path=s["path"], off=s["off"], b=b, j=j, kernel=KERNELS[(fi + 2 * j) % 5],
                     metric="l2", aniso=bool(j), noise="batch", gathered=True, bi=False, own_query=not j, yk=bool(j))
            c = _fix(c, s)
            c["gathered"] = True
            cases.append(c)
    count = {}
    for c in cases:  # (an entry of one shape may draw the same modes twice: the second is another problem of that id)
        cid = _case_id(c)
        count[cid] = count.get(cid, 0) + 1
        c["id"] = cid if count[cid] == 1 else f"{cid}-{count[cid]}"
    ids = [c["id"] for c in cases]
    assert len(set(ids)) == len(ids), sorted(i for i in ids if ids.count(i) > 1)
    return cases


def _long_cases():
    out = []
    for fi, family in enumerate(FAMILIES):
        name, dtype = family.split("/")
        entry, k, R, d = LONG[name]
        entry = entry or ("RHS4g" if dtype == "float32" else "RHS4")
        e = next(e for e in ENTRIES if e["family"] == family and e["name"] == entry)
        c = dict(entry=entry, family=family, dtype=dtype, packed=False, prefix=e["prefix"], exact=e["exact"], k=k, R=R, d=d,
                 path="auto", off=False, b=LONG_B, j=0, kernel=NO_M05[fi % 4], metric="l2", aniso=bool(fi % 2), noise="batch",
                 gathered=True, bi=False, own_query=True, yk=name not in ("rhs_mf",))
        c = _fix(c, dict(kernels=None, gathered=None, yk=None))
        c["id"] = _case_id(c)
        out.append(c)
    return out


def _entry_cases():
    """One case per entry for the non-SPD flag and the bit-for-bit agreement of the modes: batch noise, table
    responses, no batch index, a query table of its own, in the entry's first shape that gathered responses reach
    (its first shape where none does)."""
    out = []
    for i, e in enumerate(ENTRIES):
        s = next((s for s in e["shapes"] if s["gathered"] is not False), e["shapes"][0])
        c = dict(entry=e["name"], family=e["family"], dtype=e["dtype"], packed=e["packed"], prefix=e["prefix"], exact=e["exact"],
                 k=s["k"], R=s["R"], d=s["d"], path=s["path"], off=s["off"], b=B, j=i, kernel=KERNELS[i % 5], metric="l2",
                 aniso=bool(i % 2), noise="batch", gathered=False, bi=False, own_query=True, yk=True)
        c = _fix(c, dict(s, gathered=False))
        c["can_gather"] = s["gathered"] is not False
        c["id"] = "modes-" + _case_id(c)
        out.append(c)
    return out


CASES = _cases()
LONG_CASES = _long_cases()
ENTRY_CASES = _entry_cases()
BY_ID = {c["id"]: c for c in CASES + LONG_CASES + ENTRY_CASES}


def rows_of(c):
    return c["k"] + 1 + c["R"]


# ---- the problem of a case ---------------------------------------------------------------------------------------------
def _build(c, b, draw):
    rng = np.random.default_rng([SEED, sum(map(ord, c["id"])), len(c["id"]), draw])
    k, R, d = c["k"], c["R"], c["d"]
    Xn = rng.uniform(size=(N, d))
    Y = np.stack([np.sin(3.0 * Xn.sum(1) / np.sqrt(d) + r) + 0.1 * rng.normal(size=N) for r in range(R)], axis=1)
    nq = max(NQ, b)  # (no batch index: neighbourhood i reads query row i, so the long cases bring b query rows)
    Xq = rng.uniform(size=(nq, d)) if c["own_query"] else Xn
    if b <= 4096:
        ni = np.stack([rng.choice(N, size=k, replace=False) for _ in range(b)])
    else:
        ni = np.argsort(rng.uniform(size=(b, N)), axis=1)[:, :k]
    bi = rng.choice(Xq.shape[0], size=b, replace=False) if c["bi"] else np.arange(b)
    iso = float(np.sqrt(d / 6.0))
    ls = iso * (1.0 + 0.3 * rng.uniform(size=d)) if c["aniso"] else iso
    table = NOISE * (1.0 + 3.0 * rng.uniform(size=N))
    noise_rows = np.full((b, k), NOISE) if c["noise"] == "scalar" else table[ni]
    for a in (Xn, Y, Xq, ni, bi, table, noise_rows):
        a.setflags(write=False)
    return SimpleNamespace(Xn=Xn, Y=Y, Xq=Xq, ni=ni, bi=bi, ls=ls, table=table, noise_rows=noise_rows, b=b)


@functools.lru_cache(maxsize=None)
def problem(case_id):
    """The inputs of a case (read-only, shared): Xn (n, d), Y (n, R), Xq (the query table, Xn itself unless the case
    has its own), ni (b, k), bi (b,) (arange(b) where the call passes no batch index), ls (a float or (d,)), the noise
    table (n,) and the noise diagonal of every neighbourhood (b, k) whatever the layout it arrives in."""
    c = BY_ID[case_id]
    assert c["b"] <= 4096, "a long case: long_problem()"
    return _build(c, c["b"], RESEED.get(case_id, 0))


@functools.lru_cache(maxsize=1)
def long_problem(case_id):
    c = BY_ID[case_id]
    return _build(c, c["b"], 0)


# ---- the oracle, restated in a number format ---------------------------------------------------------------------------
def _covariance(kernel, x, T):
    """oracle.muygps_oracle.KERNELS on the scaled metric value ``x``, every constant in the format of ``x``."""
    if kernel == "rbf":
        return np.exp(-x / T(2))
    if kernel == "matern05":
        return np.exp(-x)
    if kernel == "matern15":
        s = x * T(np.sqrt(3.0))
        return (T(1) + s) * np.exp(-s)
    if kernel == "matern25":
        s = x * T(np.sqrt(5.0))
        return (T(1) + s + s * s / T(3)) * np.exp(-s)
    assert kernel == "maternInf", kernel
    return np.exp(-(x * x) / T(2))


def _scaled_metric(diffs, ls, metric, T):
    """Isotropy: reduce, then divide by l (l2) or l^2 (F2); Anisotropy: divide by the (d,) scales, then reduce."""
    if np.ndim(ls) == 1:
        diffs = diffs / np.asarray(ls, dtype=diffs.dtype)
    f2 = np.sum(diffs * diffs, axis=-1)
    x = np.sqrt(f2) if metric == "l2" else f2
    if np.ndim(ls) == 1:
        return x
    return x / T(ls) if metric == "l2" else x / (T(ls) * T(ls))


def covariances(c, P, dtype, rows=None, bi=None):
    """(Kin (m, k, k) WITHOUT noise, Kcross (m, k)) of the neighbourhoods ``rows`` (default: all), features rounded to
    ``dtype``, difference form, every operation in ``dtype``.  ``bi``: other query rows than the problem's."""
    T = np.dtype(dtype).type
    rows = np.arange(P.b) if rows is None else np.asarray(rows)
    bi = P.bi if bi is None else bi
    Xn, Xq = P.Xn.astype(dtype), P.Xq.astype(dtype)
    k, d = c["k"], c["d"]
    Kin = np.empty((len(rows), k, k), dtype=dtype)
    Kc = np.empty((len(rows), k), dtype=dtype)
    step = max(1, 4_000_000 // (k * k * d))
    for s in range(0, len(rows), step):
        r = rows[s:s + step]
        pts = Xn[P.ni[r]]  # (m, k, d)
        Kin[s:s + step] = _covariance(c["kernel"], _scaled_metric(pts[:, None, :, :] - pts[:, :, None, :], P.ls, c["metric"], T), T)
        Kc[s:s + step] = _covariance(c["kernel"], _scaled_metric(Xq[bi[r]][:, None, :] - pts, P.ls, c["metric"], T), T)
    assert Kin.dtype == np.dtype(dtype) and Kc.dtype == np.dtype(dtype)
    return Kin, Kc


def solve(Kin, Kc, noise_rows, Yn):
    """mean (m, R), var (m,), ykinvy (m, R) from the pieces, in their format: ``np.linalg.solve`` on K + diag(noise)
    with the right-hand sides [Kcross | Y] (the pattern of tests/test_gpu_large.py::oracle_outputs)."""
    dtype = Kin.dtype
    T = dtype.type
    K = Kin + np.stack([np.diag(r) for r in noise_rows.astype(dtype)])
    Yn = Yn.astype(dtype)
    A = np.linalg.solve(K, np.concatenate([Kc[:, :, None], Yn], axis=2))
    assert A.dtype == dtype
    mean = np.einsum("bk,bkr->br", Kc, A[:, :, 1:])
    var = T(1) - np.einsum("bk,bk->b", Kc, A[:, :, 0])
    yk = np.einsum("bkr,bkr->br", Yn, A[:, :, 1:])
    return mean, var, yk


def outputs(c, dtype, rows=None, noise_rows=None):
    """(mean (b, R), var (b,), ykinvy (b, R)) of a case by the oracle restated in ``dtype`` (np.float64: the reference;
    np.float32: what plain fp32 arithmetic makes of the same inputs).  ``rows``: a subset of the neighbourhoods;
    ``noise_rows``: another (b, k) noise diagonal than the problem's."""
    P = long_problem(c["id"]) if c["b"] > 4096 else problem(c["id"])
    sel = np.arange(P.b) if rows is None else np.asarray(rows)
    Kin, Kc = covariances(c, P, dtype, sel)
    nz = P.noise_rows if noise_rows is None else noise_rows
    return solve(Kin, Kc, nz[sel], P.Y[P.ni[sel]])


@functools.lru_cache(maxsize=None)
def reference(case_id):
    """The fp64 outputs of a case of the b <= 37 sample: computed once, read-only, shared among the tests."""
    out = outputs(BY_ID[case_id], np.float64)
    for a in out:
        a.setflags(write=False)
    return out


def band_error(got, ref):
    """The smallest t with |got - ref| <= t |ref| + t rms(ref) (tests/util.assert_close)."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    rms = float(np.sqrt(np.mean(ref**2)))
    return float(np.max(np.abs(got - ref) / (np.abs(ref) + rms)))


def rel_error(got, ref):
    """The smallest t with |got - ref| <= t |ref| (tests/util.assert_rel_close)."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.max(np.abs(got - ref) / np.abs(ref)))
