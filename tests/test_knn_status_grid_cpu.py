"""CPU: the status the k-NN entries of the C ABI return for arguments they refuse (or have nothing to do for) BEFORE any
HIP call -- the three exact scans (mgp_knn_scan_f32, mgp_knn_scan_bf16x3, mgp_knn_scan_bf16x2_d8) and the two selection
steps around them (mgp_topk_rows_f32, mgp_knn_finish_f32).  The order of the checks, read from csrc/mgp_capi.hip and
the launchers in csrc/mgp_knn.hip / csrc/mgp_knn_select.hip:

    sizes (MGP_EINVAL)  ->  [d8 entry: d > 8, MGP_EUNSUPPORTED]  ->  nothing to do (MGP_OK)  ->  NULL pointers (MGP_EINVAL)
    ->  shapes, alignment, n < 2^31, [f32 entry: start % 64] (MGP_EUNSUPPORTED)

One rule is violated per row, starting from arguments that would launch.  Host buffers stand in for device pointers:
nothing dereferences them before the status is decided.  No row here reaches a launch (and the arguments that would are
never passed as they are)."""

import ctypes as C

import pytest

from muygpys_amd import _lib

OK, EINVAL, EUNSUPPORTED = _lib.OK, _lib.EINVAL, _lib.EUNSUPPORTED

F32 = "train sqn n d q qsqn self m k start best_d best_i overflow st"
PACKED = "train ptrain sqn n d q pq qsqn self m k start best_d best_i overflow st"
ENTRIES = {
    "knn_scan_f32": F32,
    "knn_scan_bf16x3": PACKED,
    "knn_scan_bf16x2_d8": PACKED,
    "topk_rows_f32": "x rows cols stride k ov oi st",
    "knn_finish_f32": "q train d cand m k map oi od st",
}
SCANS = ("knn_scan_f32", "knn_scan_bf16x3", "knn_scan_bf16x2_d8")
NUMBERS = {
    **{e: dict(n=1000, d=8, m=5, k=3, start=64) for e in SCANS},
    "topk_rows_f32": dict(rows=3, cols=100, stride=100, k=5),
    "knn_finish_f32": dict(d=8, m=3, k=5),
}
OPTIONAL = ("self", "map", "st")  # NULL in the arguments that would launch
ALIGNED = {  # the pointers whose rows are read 16 bytes at a time
    "knn_scan_f32": "train q",
    "knn_scan_bf16x3": "train q ptrain pq",
    "knn_scan_bf16x2_d8": "train q ptrain pq",
    "knn_finish_f32": "q train",
}
_BUF = (C.c_char * 4096)()
PTR = (C.addressof(_BUF) + 15) // 16 * 16  # 16-byte aligned, like every device allocation


def status(entry, **changes):
    names = ENTRIES[entry].split()
    args = {n: NUMBERS[entry][n] if n in NUMBERS[entry] else (None if n in OPTIONAL else PTR) for n in names}
    unknown = set(changes) - set(names)
    assert not unknown, (entry, unknown)
    assert changes, "the arguments that would launch are never passed as they are"
    args.update(changes)
    return getattr(_lib.load(), f"mgp_{entry}")(*[args[n] for n in names])


def required(entry):
    return [n for n in ENTRIES[entry].split() if n not in NUMBERS[entry] and n not in OPTIONAL]


def scan_rows(entry):
    nothing = {n: None for n in ENTRIES[entry].split() if n not in NUMBERS[entry]}
    rows = [(f"{s} < 0", {s: -1}, EINVAL) for s in ("n", "m", "start")]
    rows += [("d < 1", dict(d=0), EINVAL), ("k < 1", dict(k=0), EINVAL)]
    rows += [(f"{p} NULL", {p: None}, EINVAL) for p in required(entry)]
    rows += [("no queries, all pointers NULL", dict(m=0, **nothing), OK),
             ("start = n, all pointers NULL", dict(start=1000, **nothing), OK),
             ("start > n, all pointers NULL", dict(start=1064, **nothing), OK),
             ("no queries, k < 1", dict(m=0, k=0), EINVAL)]
    rows += [("k = 65", dict(k=65), EUNSUPPORTED)]
    rows += [(f"d = {d}", dict(d=d), EUNSUPPORTED) for d in (2, 6, 68)]
    rows += [(f"{p} 4 bytes off alignment", {p: PTR + 4}, EUNSUPPORTED) for p in ALIGNED[entry].split()]
    rows += [("n = 2^31", dict(n=2**31), EUNSUPPORTED)]
    rows += [("k = 65 with a NULL pointer", dict(k=65, best_d=None), EINVAL)]  # MGP_EINVAL before MGP_EUNSUPPORTED
    if entry == "knn_scan_f32":
        rows += [("start = 2 (the norms' alignment)", dict(start=2), EUNSUPPORTED),
                 ("start = 4 (tiles off the norms' padding)", dict(start=4), EUNSUPPORTED),
                 ("start = 68", dict(start=68), EUNSUPPORTED),
                 ("start = 64, no queries", dict(start=64, m=0), OK),
                 ("start = 4, no queries", dict(start=4, m=0), OK)]  # (nothing to do comes first)
    if entry == "knn_scan_bf16x2_d8":
        rows += [("d = 12", dict(d=12), EUNSUPPORTED),
                 ("d = 12, no queries", dict(d=12, m=0), EUNSUPPORTED),  # (checked in front of the empty batch)
                 ("d = 12, no queries, all pointers NULL", dict(d=12, m=0, **nothing), EUNSUPPORTED),
                 ("d = 12, k < 1", dict(d=12, k=0), EINVAL)]
    return rows


def topk_rows():
    nothing = dict(x=None, ov=None, oi=None)
    return [
        ("rows < 0", dict(rows=-1), EINVAL), ("cols < 1", dict(cols=0), EINVAL), ("k < 1", dict(k=0), EINVAL),
        ("row_stride < cols", dict(stride=99), EINVAL),
        ("no rows, all pointers NULL", dict(rows=0, **nothing), OK),
        ("no rows, k < 1", dict(rows=0, k=0), EINVAL),
        ("no rows, k > cols", dict(rows=0, k=101, **nothing), OK),
        *[(f"{p} NULL", {p: None}, EINVAL) for p in required("topk_rows_f32")],
        ("k > cols", dict(k=101), EUNSUPPORTED),
        ("k = cols + 1 at one column", dict(cols=1, stride=1, k=2), EUNSUPPORTED),
        ("cols > 4096", dict(cols=4097, stride=4097), EUNSUPPORTED),
        ("k > cols with a NULL pointer", dict(k=101, x=None), EINVAL),
    ]


def finish_rows():
    nothing = dict(q=None, train=None, cand=None, oi=None, od=None)
    return [
        ("m < 0", dict(m=-1), EINVAL), ("d < 1", dict(d=0), EINVAL), ("k < 1", dict(k=0), EINVAL),
        ("no queries, all pointers NULL", dict(m=0, **nothing), OK),
        ("no queries, k < 1", dict(m=0, k=0), EINVAL),
        ("no queries, k > 64", dict(m=0, k=65, **nothing), OK),
        *[(f"{p} NULL", {p: None}, EINVAL) for p in required("knn_finish_f32")],
        ("k > 64", dict(k=65), EUNSUPPORTED),
        *[(f"d = {d}", dict(d=d), EUNSUPPORTED) for d in (1, 6, 10)],
        *[(f"{p} 4 bytes off alignment", {p: PTR + 4}, EUNSUPPORTED) for p in ALIGNED["knn_finish_f32"].split()],
        ("k > 64 with a NULL pointer", dict(k=65, od=None), EINVAL),
    ]


GRID = [(e, n, ch, want) for e in SCANS for n, ch, want in scan_rows(e)]
GRID += [("topk_rows_f32", n, ch, want) for n, ch, want in topk_rows()]
GRID += [("knn_finish_f32", n, ch, want) for n, ch, want in finish_rows()]


@pytest.mark.parametrize("entry, name, changes, want", GRID, ids=[f"{e}: {n}" for e, n, _, _ in GRID])
def test_status_of_refused_and_empty_calls(entry, name, changes, want):
    assert status(entry, **changes) == want


def test_the_grid_names_every_pointer():
    """The parameter lists above against the header's: as many parameters, and every pointer among them is either in a
    'NULL' row or optional."""
    for entry, names in ENTRIES.items():
        fn = getattr(_lib.load(), f"mgp_{entry}")
        assert len(fn.argtypes) == len(names.split()), entry
        for name, ctype in zip(names.split(), fn.argtypes):
            assert (name in NUMBERS[entry]) == (ctype in (C.c_int, C.c_int64)), (entry, name, ctype)
