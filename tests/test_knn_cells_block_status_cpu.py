"""CPU: the block scan of the inverted-cell index (mgp_knn_cells_scan_block) is declared in the header, and the entry
refuses bad arguments before any HIP call (in the manner of tests/test_neighbors_cells_cpu.py)."""

import ctypes

import pytest

torch = pytest.importorskip("torch")


def test_header_declares_the_block_scan():
    from muygpys_amd import _abi, _lib

    assert "mgp_knn_cells_scan_block" in _lib.exported_names_from_header()
    restype, argtypes = _abi.signatures()["mgp_knn_cells_scan_block"]
    P, I, L = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    assert restype is ctypes.c_int
    # table table_sqn n d | cell_start nlist | queries query_sqn m | probes nprobe | skip_cell self_pos | k best_d best_i
    # | overflow | stream
    assert argtypes == [P, P, L, I, P, I, P, P, L, P, I, P, P, I, P, P, P, P]


def test_block_scan_rejects_bad_arguments_without_a_gpu():
    from muygpys_amd import _lib

    lib = _lib.load()
    buf = (ctypes.c_char * 4096)()
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) // 16 * 16)  # (a host address: no accepted call is made with it)

    def call(table=p, table_sqn=p, n=1000, d=8, cell_start=p, nlist=10, queries=p, query_sqn=p, m=5, probes=p, nprobe=3,
             skip_cell=None, self_pos=None, k=10, best_d=p, best_i=p, overflow=p):
        return lib.mgp_knn_cells_scan_block(table, table_sqn, n, d, cell_start, nlist, queries, query_sqn, m, probes,
                                            nprobe, skip_cell, self_pos, k, best_d, best_i, overflow, None)

    for name in ("table", "table_sqn", "cell_start", "queries", "query_sqn", "probes", "best_d", "best_i", "overflow"):
        assert call(**{name: None}) == _lib.EINVAL, name
    assert call(k=0) == _lib.EINVAL
    assert call(nprobe=0) == _lib.EINVAL
    assert call(nprobe=11) == _lib.EINVAL  # more than nlist
    assert call(nlist=0, nprobe=1) == _lib.EINVAL
    assert call(n=-1) == _lib.EINVAL and call(m=-1) == _lib.EINVAL
    assert call(k=65) == _lib.EUNSUPPORTED
    assert call(d=6) == _lib.EUNSUPPORTED
    assert call(d=68) == _lib.EUNSUPPORTED
    assert call(n=2**31) == _lib.EUNSUPPORTED
    assert call(nlist=4097) == _lib.EUNSUPPORTED  # the union's bitmap
    misaligned = ctypes.c_void_p(p.value + 4)
    assert call(table=misaligned) == _lib.EUNSUPPORTED and call(queries=misaligned) == _lib.EUNSUPPORTED
    # sizes are looked at before pointers, and an empty batch reads nothing
    assert call(table=None, k=65) == _lib.EUNSUPPORTED
    assert call(table=None, queries=None, m=0) == _lib.OK
