"""CPU: the status the long-row k-NN entries of the C ABI (mgp_knn_scan_long, mgp_knn_scan_long_wide: rows of 68 to
256 features, csrc/mgp_knn_long.hip) return for arguments they refuse, or have nothing to do for, BEFORE any HIP call,
and the route rule of NN_Wrapper (muygpys_amd.neighbors.scan_route), which needs no device.  The order of the checks
(include/muygpys_hip.h), that of the entries they mirror:

    sizes (MGP_EINVAL)  ->  nothing to do (MGP_OK, pointers not looked at)  ->  NULL pointers (MGP_EINVAL)
    ->  k > 64 (1024), d outside {68, 72, .. 256}, alignment, n >= 2^31, start % 64, and for the wide entry
        k (+ 1 with self_idx) > start (MGP_EUNSUPPORTED)

One rule is violated per row, starting from arguments that would launch (built as in tests/test_knn_wide_status_cpu.py).
Host buffers stand in for device pointers: nothing dereferences them before the status is decided.  No row here reaches
a launch (and the arguments that would are never passed as they are)."""

import ctypes as C

import pytest

from muygpys_amd import _lib

OK, EINVAL, EUNSUPPORTED = _lib.OK, _lib.EINVAL, _lib.EUNSUPPORTED

PARAMS = "train sqn n d q qsqn self m k start best_d best_i overflow st"
ENTRIES = ("knn_scan_long", "knn_scan_long_wide")
NUMBERS = {
    "knn_scan_long": dict(n=5000, d=100, m=5, k=30, start=128),
    "knn_scan_long_wide": dict(n=5000, d=100, m=5, k=100, start=128),
    # (the old entries, at the same arguments: asked only for what they go on refusing)
    "knn_scan_f32": dict(n=5000, d=100, m=5, k=30, start=128),
    "knn_scan_wide": dict(n=5000, d=100, m=5, k=100, start=128),
}
MAX_K = {"knn_scan_long": 64, "knn_scan_long_wide": 1024}
TWIN = {"knn_scan_long": "mgp_knn_scan_f32", "knn_scan_long_wide": "mgp_knn_scan_wide"}
OPTIONAL = ("self", "st")  # NULL in the arguments that would launch
_BUF = (C.c_char * 4096)()
PTR = (C.addressof(_BUF) + 15) // 16 * 16  # 16-byte aligned, like every device allocation


def status(entry, **changes):
    names = PARAMS.split()
    args = {n: NUMBERS[entry][n] if n in NUMBERS[entry] else (None if n in OPTIONAL else PTR) for n in names}
    unknown = set(changes) - set(names)
    assert not unknown, (entry, unknown)
    assert changes, "the arguments that would launch are never passed as they are"
    args.update(changes)
    return getattr(_lib.load(), f"mgp_{entry}")(*[args[n] for n in names])


def required(entry):
    return [n for n in PARAMS.split() if n not in NUMBERS[entry] and n not in OPTIONAL]


def scan_rows(entry):
    kmax = MAX_K[entry]
    nothing = {n: None for n in PARAMS.split() if n not in NUMBERS[entry]}
    rows = [(f"{s} < 0", {s: -1}, EINVAL) for s in ("n", "m", "start")]
    rows += [("d < 1", dict(d=0), EINVAL), ("k < 1", dict(k=0), EINVAL)]
    rows += [("no queries, all pointers NULL", dict(m=0, **nothing), OK),
             ("start = n, all pointers NULL", dict(start=5000, **nothing), OK),
             ("start > n, all pointers NULL", dict(start=5056, **nothing), OK),
             ("no queries, k < 1", dict(m=0, k=0), EINVAL),
             (f"no queries, k = {kmax + 1}", dict(m=0, k=kmax + 1, **nothing), OK),
             ("no queries, d = 64", dict(m=0, d=64, **nothing), OK),
             ("start = 4, no queries", dict(start=4, m=0), OK)]  # (nothing to do comes first)
    rows += [(f"{p} NULL", {p: None}, EINVAL) for p in required(entry)]
    rows += [(f"k = {kmax + 1}", dict(k=kmax + 1, start=2048), EUNSUPPORTED),
             (f"k = {kmax + 1} with a NULL pointer", dict(k=kmax + 1, start=2048, best_d=None), EINVAL)]  # EINVAL first
    rows += [(f"d = {d}", dict(d=d), EUNSUPPORTED) for d in (4, 40, 64, 66, 70, 260)]
    rows += [(f"{p} 4 bytes off alignment", {p: PTR + 4}, EUNSUPPORTED) for p in ("train", "q")]
    rows += [("n = 2^31", dict(n=2**31), EUNSUPPORTED)]
    rows += [("start = 130 (the norms' alignment)", dict(start=130), EUNSUPPORTED),
             ("start = 132 (tiles off the norms' padding)", dict(start=132), EUNSUPPORTED)]
    if entry == "knn_scan_long_wide":
        # the IN lists must be whole: k rows below start, k + 1 where a self row may be one of them
        rows += [("k = start + 1", dict(k=129), EUNSUPPORTED),
                 ("k = start with self_idx", dict(k=128, self=PTR), EUNSUPPORTED),
                 ("k = 1024 at start = 1024 with self_idx", dict(k=1024, start=1024, self=PTR), EUNSUPPORTED),
                 ("k = 65 at start = 64", dict(k=65, start=64), EUNSUPPORTED)]
    else:
        rows += [("k = 65", dict(k=65), EUNSUPPORTED)]
    return [(entry, *row) for row in rows]


# the entries for d <= 64 keep refusing longer rows, whatever else is right (their own grids:
# tests/test_knn_status_grid_cpu.py, tests/test_knn_wide_status_cpu.py)
OLD = [(e, f"d = {d}", dict(d=d), EUNSUPPORTED) for e in ("knn_scan_f32", "knn_scan_wide") for d in (68, 100, 256)]

GRID = [row for entry in ENTRIES for row in scan_rows(entry)] + OLD


@pytest.mark.parametrize("entry, name, changes, want", GRID, ids=[f"{e}: {n}" for e, n, _, _ in GRID])
def test_status_of_refused_and_empty_calls(entry, name, changes, want):
    assert status(entry, **changes) == want


def test_the_packed_entries_refuse_long_rows_too():
    lib = _lib.load()
    for name in ("mgp_knn_scan_bf16x3", "mgp_knn_scan_bf16x2_d8"):
        rc = getattr(lib, name)(PTR, PTR, PTR, 5000, 68, PTR, PTR, PTR, None, 5, 30, 128, PTR, PTR, PTR, None)
        assert rc == EUNSUPPORTED, name


def test_the_widest_row():
    assert _lib.load().mgp_knn_long_max_features() == 256
    from muygpys_amd import neighbors

    assert neighbors.LONG_MAX_D == 256


def test_the_header_declares_the_three_names():
    names = _lib.exported_names_from_header()
    for name in ("mgp_knn_long_max_features", "mgp_knn_scan_long", "mgp_knn_scan_long_wide"):
        assert name in names, name
        assert hasattr(_lib.load(), name), name


@pytest.mark.parametrize("entry", ENTRIES)
def test_signatures_equal_the_entries_they_mirror(entry):
    lib = _lib.load()
    new, old = getattr(lib, f"mgp_{entry}"), getattr(lib, TWIN[entry])
    assert list(new.argtypes) == list(old.argtypes)
    assert new.restype == old.restype
    assert len(new.argtypes) == len(PARAMS.split())
    for name, ctype in zip(PARAMS.split(), new.argtypes):
        assert (name in NUMBERS[entry]) == (ctype in (C.c_int, C.c_int64)), (entry, name, ctype)


# ---- the route rule ------------------------------------------------------------------------------------------------
torch = pytest.importorskip("torch")
F32, F64, N = torch.float32, torch.float64, 9001
NO_ENV = {}
ROUTES = [
    # d, k, dtype, rows, use_scan, environment, route
    (1, 10, F32, N, True, NO_ENV, "scan"), (3, 10, F32, N, True, NO_ENV, "scan"), (4, 10, F32, N, True, NO_ENV, "scan"),
    (63, 10, F32, N, True, NO_ENV, "scan"), (64, 10, F32, N, True, NO_ENV, "scan"), (64, 64, F32, N, True, NO_ENV, "scan"),
    (1, 65, F32, N, True, NO_ENV, "wide"), (3, 1024, F32, N, True, NO_ENV, "wide"), (64, 65, F32, N, True, NO_ENV, "wide"),
    (65, 10, F32, N, True, NO_ENV, "long"), (68, 10, F32, N, True, NO_ENV, "long"), (68, 65, F32, N, True, NO_ENV, "long"),
    (100, 30, F32, N, True, NO_ENV, "long"), (253, 64, F32, N, True, NO_ENV, "long"), (256, 1024, F32, N, True, NO_ENV, "long"),
    (257, 10, F32, N, True, NO_ENV, None), (260, 10, F32, N, True, NO_ENV, None), (1000, 10, F32, N, True, NO_ENV, None),
    (64, 1025, F32, N, True, NO_ENV, None), (256, 1025, F32, N, True, NO_ENV, None), (40, 0, F32, N, True, NO_ENV, None),
    (40, 10, F64, N, True, NO_ENV, None), (100, 10, F64, N, True, NO_ENV, None), (3, 10, F64, N, True, NO_ENV, None),
    (40, 10, F32, 8192, True, NO_ENV, None), (100, 10, F32, 8192, True, NO_ENV, None), (40, 10, F32, 8193, True, NO_ENV, "scan"),
    (100, 10, F32, 2**31, True, NO_ENV, None), (100, 10, F32, 2**31 - 1, True, NO_ENV, "long"),
    (40, 10, F32, N, False, NO_ENV, None), (100, 10, F32, N, False, NO_ENV, None), (3, 10, F32, N, False, NO_ENV, None),
    # the switches: each one keeps its own shapes dense and nothing else
    (40, 65, F32, N, True, {"MUYGPYS_HIP_KNN_WIDE": "0"}, None), (100, 65, F32, N, True, {"MUYGPYS_HIP_KNN_WIDE": "0"}, None),
    (40, 64, F32, N, True, {"MUYGPYS_HIP_KNN_WIDE": "0"}, "scan"), (100, 64, F32, N, True, {"MUYGPYS_HIP_KNN_WIDE": "0"}, "long"),
    (68, 10, F32, N, True, {"MUYGPYS_HIP_KNN_LONG": "0"}, None), (65, 10, F32, N, True, {"MUYGPYS_HIP_KNN_LONG": "0"}, None),
    (64, 10, F32, N, True, {"MUYGPYS_HIP_KNN_LONG": "0"}, "scan"), (63, 65, F32, N, True, {"MUYGPYS_HIP_KNN_LONG": "0"}, "wide"),
    (1, 10, F32, N, True, {"MUYGPYS_HIP_KNN_PAD": "0"}, None), (3, 65, F32, N, True, {"MUYGPYS_HIP_KNN_PAD": "0"}, None),
    (63, 10, F32, N, True, {"MUYGPYS_HIP_KNN_PAD": "0"}, None), (65, 10, F32, N, True, {"MUYGPYS_HIP_KNN_PAD": "0"}, None),
    (4, 10, F32, N, True, {"MUYGPYS_HIP_KNN_PAD": "0"}, "scan"), (68, 10, F32, N, True, {"MUYGPYS_HIP_KNN_PAD": "0"}, "long"),
    (100, 10, F32, N, True, {"MUYGPYS_HIP_KNN_LONG": "1", "MUYGPYS_HIP_KNN_PAD": "1"}, "long"),
]


@pytest.mark.parametrize("d, k, dtype, n, use_scan, env, want", ROUTES,
                         ids=[f"d{d}-k{k}-{str(t)[6:]}-n{n}-scan{int(u)}-{'+'.join(f'{a[16:]}={b}' for a, b in e.items()) or 'default'}"
                              for d, k, t, n, u, e, _ in ROUTES])
def test_scan_route(d, k, dtype, n, use_scan, env, want, monkeypatch):
    from muygpys_amd.neighbors import scan_route, stored_width

    for name in ("MUYGPYS_HIP_KNN_WIDE", "MUYGPYS_HIP_KNN_LONG", "MUYGPYS_HIP_KNN_PAD"):
        monkeypatch.delenv(name, raising=False)
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    assert scan_route(d, k, dtype, n, use_scan) == want
    assert stored_width(d) == max(4, (d + 3) // 4 * 4)
