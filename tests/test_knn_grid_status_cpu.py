"""CPU: the status mgp_knn_grid_scan (the grid walk of the exact search at 1 to 3 features, csrc/mgp_knn_grid.hip) returns
for arguments it refuses, or has nothing to do for, BEFORE any HIP call.  The order of the checks (include/muygpys_hip.h):

    sizes (MGP_EINVAL)  ->  nothing to do (MGP_OK, pointers not looked at)  ->  NULL pointers (MGP_EINVAL)
    ->  k > 64, n >= 2^31, g0 g1 g2 > 2^24, alignment, a launch grid of 2^31 workgroups (MGP_EUNSUPPORTED)

One rule is violated per row, starting from arguments that would launch.  Host buffers stand in for device pointers:
nothing dereferences them before the status is decided.  No row here reaches a launch (and the arguments that would are
never passed as they are)."""

import ctypes as C

import pytest

from muygpys_amd import _abi, _lib

OK, EINVAL, EUNSUPPORTED = _lib.OK, _lib.EINVAL, _lib.EUNSUPPORTED

NAMES = "table n cell_start g0 g1 g2 edges q m qcell self k best_d best_i shells st".split()
NUMBERS = dict(n=5000, g0=10, g1=5, g2=2, m=5, k=30)
OPTIONAL = ("self", "st")  # NULL in the arguments that would launch
_BUF = (C.c_char * 4096)()
PTR = (C.addressof(_BUF) + 15) // 16 * 16  # 16-byte aligned, like every device allocation


def status(**changes):
    args = {n: NUMBERS[n] if n in NUMBERS else (None if n in OPTIONAL else PTR) for n in NAMES}
    unknown = set(changes) - set(NAMES)
    assert not unknown, unknown
    assert changes, "the arguments that would launch are never passed as they are"
    args.update(changes)
    return _lib.load().mgp_knn_grid_scan(*[args[n] for n in NAMES])


REQUIRED = [n for n in NAMES if n not in NUMBERS and n not in OPTIONAL and n != "edges"]
NOTHING = {n: None for n in NAMES if n not in NUMBERS}

ROWS = [
    *[(f"{s} < 0", {s: -1}, EINVAL) for s in ("n", "m")],
    ("k < 1", dict(k=0), EINVAL),
    *[(f"{g} < 1", {g: 0}, EINVAL) for g in ("g0", "g1", "g2")],
    ("no queries, all pointers NULL", dict(m=0, **NOTHING), OK),
    ("no queries, k < 1", dict(m=0, k=0), EINVAL),                      # (sizes come first)
    ("no queries, k = 65, all pointers NULL", dict(m=0, k=65, **NOTHING), OK),  # (nothing to do comes before the limits)
    ("no queries, 2^30 cells", dict(m=0, g0=1024, g1=1024, g2=1024), OK),
    *[(f"{p} NULL", {p: None}, EINVAL) for p in REQUIRED],
    ("edges NULL on a grid with edges", dict(edges=None), EINVAL),
    ("edges NULL, only g2 > 1", dict(edges=None, g0=1, g1=1), EINVAL),
    ("k = 65", dict(k=65), EUNSUPPORTED),
    ("k = 65 with a NULL pointer", dict(k=65, best_d=None), EINVAL),     # (EINVAL comes first)
    ("n = 2^31", dict(n=2**31), EUNSUPPORTED),
    ("2^24 + 1 cells in one row", dict(g0=2**24 + 1, g1=1, g2=1), EUNSUPPORTED),
    ("2^24 + 2^12 cells", dict(g0=2**12, g1=2**12 + 1, g2=1), EUNSUPPORTED),
    ("2^93 cells (no overflow)", dict(g0=2**31 - 1, g1=2**31 - 1, g2=2**31 - 1), EUNSUPPORTED),
    ("2^62 cells (no overflow)", dict(g0=1, g1=2**31 - 1, g2=2**31 - 1), EUNSUPPORTED),
    ("table 4 bytes off alignment", dict(table=PTR + 4), EUNSUPPORTED),
    ("queries 4 bytes off alignment", dict(q=PTR + 4), EUNSUPPORTED),
    ("a launch grid of 2^31 workgroups", dict(m=4 * 2**31 - 3), EUNSUPPORTED),
]


@pytest.mark.parametrize("name, changes, want", ROWS, ids=[r[0] for r in ROWS])
def test_status_of_refused_and_empty_calls(name, changes, want):
    assert status(**changes) == want


def test_the_header_declares_the_entry_and_the_library_binds_it():
    assert "mgp_knn_grid_scan" in _lib.exported_names_from_header()
    assert hasattr(_lib.load(), "mgp_knn_grid_scan")
    restype, argtypes = _abi.signatures()["mgp_knn_grid_scan"]
    P, I, L = C.c_void_p, C.c_int, C.c_int64
    assert restype is C.c_int
    # table n | cell_start g0 g1 g2 | edges | queries m | qcell | self_pos | k best_d best_i | shells | stream
    assert argtypes == [P, L, P, I, I, I, P, P, L, P, P, I, P, P, P, P]


def test_the_grid_names_every_pointer():
    """The parameter list above against the header's: as many parameters, and every pointer among them is either in a
    'NULL' row or optional."""
    fn = _lib.load().mgp_knn_grid_scan
    assert len(fn.argtypes) == len(NAMES)
    for name, ctype in zip(NAMES, fn.argtypes):
        assert (name in NUMBERS) == (ctype in (C.c_int, C.c_int64)), (name, ctype)
    assert set(REQUIRED) | {"edges"} | set(OPTIONAL) == {n for n in NAMES if n not in NUMBERS}


def test_the_limits_of_the_python_route_are_the_entry_s():
    from muygpys_amd import neighbors

    assert neighbors.GRID_MAX_CELLS == 2**24 and neighbors.GRID_MAX_D == 3
    assert status(g0=2**24, g1=1, g2=1, m=0) == OK
