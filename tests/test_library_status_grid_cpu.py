"""CPU: the status every fused entry point of the C ABI returns for arguments it refuses (or has nothing to do for)
BEFORE any HIP call -- include/muygpys_hip.h: MGP_EINVAL for a null pointer / bad size / unknown enum, MGP_OK for an
empty batch (sizes are checked first; pointers and enum ids are not looked at), MGP_EUNSUPPORTED from
mgp_posterior_gen_* for a smoothness beyond 30 once everything else is in order.

One rule is violated per row, starting from arguments that would launch.  Host buffers stand in for device pointers:
nothing dereferences them before the status is decided.  No row here reaches a launch."""

import ctypes as C

import pytest

from muygpys_amd import _lib

OK, EINVAL, EUNSUPPORTED = 0, -1, -2

# parameter order of every entry (include/muygpys_hip.h)
COMMON = "nm eps nd kid mid ls lsc"
ENTRIES = {
    "posterior": f"fq fn d bi ni b k tg R {COMMON} mean var yk info st",
    "posterior_gathered": f"fq fn d bi ni b k tg R {COMMON} mean var yk info st",
    "posterior_packed": f"pq qs pn ns d bi ni b k R {COMMON} mean var yk info st",
    "posterior_packed_gathered": f"pq qs pn ns d bi ni b k tg R {COMMON} mean var yk info st",
    "posterior_gen": "fq fn pq qs pn ns d bi ni b k tg R tb nm eps nd nu mid ls lsc mean var yk info st",
    "fast_coefficients": f"fn d ni b k tg {COMMON} coeffs info st",
    "fast_posterior_mean": "fq fn d bi ni b k coeffs crow R kid mid ls lsc mean st",
    "posterior_backward": f"fq fn d bi ni b k tg R {COMMON} gmean gvar gfq gfn gtg gls gnz info st",
    "loocv": f"fn d bi ni b k tg {COMMON} mean var yk info hd partials scratch st",
    "loocv_backward": f"fn d bi ni b k tg {COMMON} gmean gvar gyk gls gnz info st",
}
NUMBERS = dict(d=4, b=3, k=5, R=1, nm=0, eps=1e-3, kid=2, mid=0, lsc=1, qs=64, ns=64, tb=0, nu=1.5, hd=1.5)
OPTIONAL = ("nd", "st")  # NULL in the arguments that would launch (scalar noise, the default stream)
# the pointers an entry cannot do without (a missing prepared neighbour table makes the call a plain-table one, whose
# feature tables are then missing)
REQUIRED = {
    "posterior": "fq fn tg ni ls mean var",
    "posterior_gathered": "fq fn tg ni ls mean var",
    "posterior_packed": "pq pn ni ls mean var",
    "posterior_packed_gathered": "pq pn tg ni ls mean var",
    "posterior_gen": "fq fn tg ni ls mean var",
    "fast_coefficients": "fn ni tg ls coeffs",
    "fast_posterior_mean": "fq fn ni coeffs crow ls mean",
    "posterior_backward": "fq fn ni tg ls",
    "loocv": "fn ni tg ls mean var yk partials scratch",
    "loocv_backward": "fn ni tg ls gmean gvar gyk",
}
BUF = (C.c_double * 64)()
PTR = C.addressof(BUF)


def status(entry, suf, **changes):
    names = ENTRIES[entry].split()
    args = {n: NUMBERS[n] if n in NUMBERS else (None if n in OPTIONAL else PTR) for n in names}
    if entry == "posterior_gen" and "pn" not in changes:
        args.update(pq=None, pn=None, qs=0, ns=0)  # (the plain-table form unless a row asks for the prepared one)
    unknown = set(changes) - set(names)
    assert not unknown, (entry, unknown)
    args.update(changes)
    return getattr(_lib.load(), f"mgp_{entry}_{suf}")(*[args[n] for n in names])


def rows_of(entry):
    """[(row name, changed arguments, expected status)] of one entry."""
    names = ENTRIES[entry].split()
    has = lambda *ns: all(n in names for n in ns)  # noqa: E731
    rows = [("b < 0", dict(b=-1), EINVAL), ("k < 1", dict(k=0), EINVAL), ("d < 1", dict(d=0), EINVAL)]
    if has("R"):
        rows.append(("R < 1", dict(R=0), EINVAL))
    rows += [(f"{p} NULL", {p: None}, EINVAL) for p in REQUIRED[entry].split()]
    if has("kid"):
        rows += [(f"kernel id {i}", dict(kid=i), EINVAL) for i in (-1, 5, 99)]  # (5: the general form has its own entry)
    rows += [(f"metric id {i}", dict(mid=i), EINVAL) for i in (-1, 2)]
    if has("nm"):
        rows += [(f"noise mode {i}", dict(nm=i), EINVAL) for i in (-1, 3)]
        rows += [(f"noise mode {i} without noise_dev", dict(nm=i, nd=None), EINVAL) for i in (1, 2)]
    rows += [(f"ls_count {i} at d = 4", dict(lsc=i), EINVAL) for i in (0, 2, 5)]
    # the empty batch: MGP_OK with nothing else in order -- but only behind the sizes
    nothing = {n: None for n in names if n not in NUMBERS}
    if entry == "loocv":  # (its sums and scratch are checked in front, also for an empty shard)
        rows.append(("empty batch, all pointers NULL", dict(b=0, **nothing), EINVAL))
    else:
        rows.append(("empty batch, all pointers NULL", dict(b=0, **nothing), OK))
        ids = dict(mid=7, lsc=9, **({"kid": 99} if has("kid") else {}), **({"nm": 8} if has("nm") else {}))
        rows.append(("empty batch, ids not looked at", dict(b=0, **nothing, **ids), OK))
    rows.append(("empty batch, k < 1", dict(b=0, k=0), EINVAL))
    return rows


ES = {"f32": 4, "f64": 8}
GRID = [(e, n, ch, want) for e in ENTRIES for n, ch, want in rows_of(e)]


@pytest.mark.parametrize("suf", ["f32", "f64"])
@pytest.mark.parametrize("entry, name, changes, want", GRID, ids=[f"{e}: {n}" for e, n, _, _ in GRID])
def test_status_of_refused_and_empty_calls(entry, name, changes, want, suf):
    assert status(entry, suf, **changes) == want


@pytest.mark.parametrize("suf", ["f32", "f64"])
def test_prepared_table_strides(suf):
    """Both strides cover the features and the 16-byte response slot; the neighbour table also the responses, unless
    they come gathered."""
    es = ES[suf]
    need = 4 * es + 16
    for entry in ("posterior_packed", "posterior_packed_gathered", "posterior_gen"):
        form = dict(pq=PTR, pn=PTR, qs=64, ns=64, fq=None, fn=None) if entry == "posterior_gen" else {}
        assert status(entry, suf, **{**form, "qs": need - 1}) == EINVAL, entry
        assert status(entry, suf, **{**form, "ns": need - 1}) == EINVAL, entry
        assert status(entry, suf, **{**form, "pq": None}) == EINVAL, entry
    # eight responses: (d + R) * es = 12 es bytes, above the 4 es + 16 of the features and the slot
    assert need <= 12 * es - 1
    assert status("posterior_packed", suf, R=8, ns=12 * es - 1) == EINVAL
    assert status("posterior_gen", suf, pq=PTR, pn=PTR, qs=64, ns=12 * es - 1, fq=None, fn=None, tg=None, R=8) == EINVAL
    # gathered responses next to prepared tables: the tensor must be there
    assert status("posterior_gen", suf, pq=PTR, pn=PTR, qs=64, ns=64, fq=None, fn=None, tg=None, tb=1) == EINVAL


@pytest.mark.parametrize("suf", ["f32", "f64"])
def test_general_smoothness_statuses_in_order(suf):
    assert status("posterior_gen", suf, nu=0.0) == EINVAL
    assert status("posterior_gen", suf, nu=-1.0) == EINVAL
    assert status("posterior_gen", suf, nu=float("nan")) == EINVAL
    assert status("posterior_gen", suf, nu=0.0, b=0) == EINVAL         # the sign is checked with the sizes
    assert status("posterior_gen", suf, nu=31.0) == EUNSUPPORTED       # everything else in order
    assert status("posterior_gen", suf, nu=31.0, pq=PTR, pn=PTR, qs=64, ns=64, fq=None, fn=None) == EUNSUPPORTED
    assert status("posterior_gen", suf, nu=31.0, b=0) == OK            # ... but an empty batch is done first
    for bad in (dict(mid=2), dict(lsc=2), dict(nm=3), dict(ls=None), dict(var=None), dict(nm=1)):
        assert status("posterior_gen", suf, nu=31.0, **bad) == EINVAL, bad  # MGP_EINVAL before MGP_EUNSUPPORTED


@pytest.mark.parametrize("suf", ["f32", "f64"])
def test_checks_of_single_entries(suf):
    # a backward call without any cotangent (grad_ykinvy is not reachable through mgp_posterior_backward_*, and
    # mgp_loocv_backward_* fixes R = 1, so "grad_ykinvy with R != 1" cannot be asked through the ABI)
    assert status("posterior_backward", suf, gmean=None, gvar=None) == EINVAL
    assert status("loocv_backward", suf, gls=None, gnz=None) == EINVAL
    assert status("loocv_backward", suf, b=0, gmean=None, gvar=None, gyk=None, gls=None, gnz=None) == OK
    for hd in (0.0, -1.0, float("nan")):
        assert status("loocv", suf, hd=hd) == EINVAL
    assert status("loocv", suf, b=0, partials=None) == EINVAL
    assert status("loocv", suf, b=0, scratch=None) == EINVAL
