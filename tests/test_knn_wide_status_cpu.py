"""CPU: the status the wide k-NN entries of the C ABI (mgp_knn_scan_wide, mgp_knn_finish_wide: lists of up to 1 024
entries, csrc/mgp_knn_wide.hip) return for arguments they refuse, or have nothing to do for, BEFORE any HIP call.  The
order of the checks (include/muygpys_hip.h):

    sizes (MGP_EINVAL)  ->  nothing to do (MGP_OK, pointers not looked at)  ->  NULL pointers (MGP_EINVAL)
    ->  k > 1024, d, alignment, n >= 2^31, start % 64, k (+ 1 with self_idx) > start (MGP_EUNSUPPORTED)

One rule is violated per row, starting from arguments that would launch.  Host buffers stand in for device pointers:
nothing dereferences them before the status is decided.  No row here reaches a launch (and the arguments that would are
never passed as they are)."""

import ctypes as C

import pytest

from muygpys_amd import _lib

OK, EINVAL, EUNSUPPORTED = _lib.OK, _lib.EINVAL, _lib.EUNSUPPORTED

ENTRIES = {
    "knn_scan_wide": "train sqn n d q qsqn self m k start best_d best_i overflow st",
    "knn_finish_wide": "q train d cand m k map oi od st",
}
NUMBERS = {
    "knn_scan_wide": dict(n=5000, d=8, m=5, k=100, start=128),
    "knn_finish_wide": dict(d=8, m=3, k=100),
}
TWIN = {"knn_scan_wide": "mgp_knn_scan_f32", "knn_finish_wide": "mgp_knn_finish_f32"}
OPTIONAL = ("self", "map", "st")  # NULL in the arguments that would launch
ALIGNED = {"knn_scan_wide": "train q", "knn_finish_wide": "q train"}
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


def scan_rows():
    entry = "knn_scan_wide"
    nothing = {n: None for n in ENTRIES[entry].split() if n not in NUMBERS[entry]}
    rows = [(f"{s} < 0", {s: -1}, EINVAL) for s in ("n", "m", "start")]
    rows += [("d < 1", dict(d=0), EINVAL), ("k < 1", dict(k=0), EINVAL)]
    rows += [("no queries, all pointers NULL", dict(m=0, **nothing), OK),
             ("start = n, all pointers NULL", dict(start=5000, **nothing), OK),
             ("start > n, all pointers NULL", dict(start=5056, **nothing), OK),
             ("no queries, k < 1", dict(m=0, k=0), EINVAL),
             ("no queries, k = 1025", dict(m=0, k=1025, **nothing), OK),
             ("start = 4, no queries", dict(start=4, m=0), OK)]  # (nothing to do comes first)
    rows += [(f"{p} NULL", {p: None}, EINVAL) for p in required(entry)]
    rows += [("k = 1025", dict(k=1025, start=2048), EUNSUPPORTED),
             ("k = 1025 with a NULL pointer", dict(k=1025, start=2048, best_d=None), EINVAL)]  # EINVAL comes first
    rows += [(f"d = {d}", dict(d=d), EUNSUPPORTED) for d in (2, 6, 68)]
    rows += [(f"{p} 4 bytes off alignment", {p: PTR + 4}, EUNSUPPORTED) for p in ALIGNED[entry].split()]
    rows += [("n = 2^31", dict(n=2**31), EUNSUPPORTED)]
    rows += [("start = 130 (the norms' alignment)", dict(start=130), EUNSUPPORTED),
             ("start = 132 (tiles off the norms' padding)", dict(start=132), EUNSUPPORTED)]
    # the IN lists must be whole: k rows below start, k + 1 where a self row may be one of them
    rows += [("k = start + 1", dict(k=129), EUNSUPPORTED),
             ("k = start with self_idx", dict(k=128, self=PTR), EUNSUPPORTED),
             ("k = 1024 at start = 1024 with self_idx", dict(k=1024, start=1024, self=PTR), EUNSUPPORTED),
             ("k = 65 at start = 64", dict(k=65, start=64), EUNSUPPORTED)]
    return [(entry, *row) for row in rows]


def finish_rows():
    entry = "knn_finish_wide"
    nothing = dict(q=None, train=None, cand=None, oi=None, od=None)
    rows = [
        ("m < 0", dict(m=-1), EINVAL), ("d < 1", dict(d=0), EINVAL), ("k < 1", dict(k=0), EINVAL),
        ("no queries, all pointers NULL", dict(m=0, **nothing), OK),
        ("no queries, k < 1", dict(m=0, k=0), EINVAL),
        ("no queries, k > 1024", dict(m=0, k=1025, **nothing), OK),
        *[(f"{p} NULL", {p: None}, EINVAL) for p in required(entry)],
        ("k > 1024", dict(k=1025), EUNSUPPORTED),
        *[(f"d = {d}", dict(d=d), EUNSUPPORTED) for d in (1, 6, 10)],
        *[(f"{p} 4 bytes off alignment", {p: PTR + 4}, EUNSUPPORTED) for p in ALIGNED[entry].split()],
        ("k > 1024 with a NULL pointer", dict(k=1025, od=None), EINVAL),
    ]
    return [(entry, *row) for row in rows]


GRID = scan_rows() + finish_rows()


@pytest.mark.parametrize("entry, name, changes, want", GRID, ids=[f"{e}: {n}" for e, n, _, _ in GRID])
def test_status_of_refused_and_empty_calls(entry, name, changes, want):
    assert status(entry, **changes) == want


def test_the_largest_list():
    assert _lib.load().mgp_knn_wide_max_nn_count() == 1024
    from muygpys_amd import neighbors

    assert neighbors.WIDE_MAX_K == 1024


def test_the_header_declares_the_three_names():
    names = _lib.exported_names_from_header()
    for name in ("mgp_knn_wide_max_nn_count", "mgp_knn_scan_wide", "mgp_knn_finish_wide"):
        assert name in names, name
        assert hasattr(_lib.load(), name), name


@pytest.mark.parametrize("entry", sorted(TWIN))
def test_signatures_equal_the_narrow_entries(entry):
    lib = _lib.load()
    wide, narrow = getattr(lib, f"mgp_{entry}"), getattr(lib, TWIN[entry])
    assert list(wide.argtypes) == list(narrow.argtypes)
    assert wide.restype == narrow.restype


def test_the_wide_kernels_use_no_scratch():
    """The build's register report (lib/kernel_resources.json): every instantiation of the two kernels is there, none
    spills a vector register and none has a stack."""
    import json
    import os

    with open(os.path.join(os.path.dirname(_lib.__file__), "lib", "kernel_resources.json")) as f:
        report = json.load(f)
    scans = {name: r for name, r in report.items() if "knn_scan_wide_kernel" in name}
    finish = {name: r for name, r in report.items() if "knn_finish_wide_kernel" in name}
    assert len(scans) == 8 and len(finish) == 1, (sorted(scans), sorted(finish))
    for name, r in {**scans, **finish}.items():
        assert r["VGPRs Spill"] == 0 and r["ScratchSize [bytes/lane]"] == 0 and r["Dynamic Stack"] == "False", (name, r)


def test_the_grid_names_every_pointer():
    """The parameter lists above against the header's: as many parameters, and every pointer among them is either in a
    'NULL' row or optional."""
    for entry, names in ENTRIES.items():
        fn = getattr(_lib.load(), f"mgp_{entry}")
        assert len(fn.argtypes) == len(names.split()), entry
        for name, ctype in zip(names.split(), fn.argtypes):
            assert (name in NUMBERS[entry]) == (ctype in (C.c_int, C.c_int64)), (entry, name, ctype)
