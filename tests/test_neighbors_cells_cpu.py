"""CPU: the pieces of the inverted-cell index (nn_method="ivf") that need no GPU -- the storage layout of an assignment
vector, the default cell counts, and the C entry's refusals before any HIP call."""

import ctypes

import pytest

torch = pytest.importorskip("torch")


def test_layout_is_a_stable_sort_by_cell():
    from muygpys_amd.neighbors import cell_layout

    #                          row: 0  1  2  3  4  5  6  7  8  9
    assignment = torch.tensor([3, 1, 3, 5, 1, 1, 6, 3, 5, 1])  # cells 0, 2, 4 and 7 are empty (first and last too)
    perm, inv, cell_start = cell_layout(assignment, 8)
    assert perm.tolist() == [1, 4, 5, 9, 0, 2, 7, 3, 8, 6]  # by cell, rows in their own order within a cell
    assert cell_start.dtype == torch.int64
    assert cell_start.tolist() == [0, 0, 4, 4, 7, 7, 9, 10, 10]
    assert inv[perm].tolist() == list(range(10)) and perm[inv].tolist() == list(range(10))
    for j in range(8):
        assert (assignment[perm[cell_start[j]:cell_start[j + 1]]] == j).all()


def test_layout_of_random_assignments():
    from muygpys_amd.neighbors import cell_layout

    g = torch.Generator().manual_seed(3)
    for n, nlist in ((1, 1), (1, 5), (1000, 7), (5000, 300)):
        assignment = torch.randint(0, nlist, (n,), generator=g)
        perm, inv, cell_start = cell_layout(assignment, nlist)
        assert cell_start.shape == (nlist + 1,) and int(cell_start[0]) == 0 and int(cell_start[-1]) == n
        assert bool((cell_start[1:] >= cell_start[:-1]).all())
        assert torch.equal(perm.sort().values, torch.arange(n))
        assert torch.equal(inv[perm], torch.arange(n))
        stored = assignment[perm]
        assert bool((stored[1:] >= stored[:-1]).all())
        same = stored[1:] == stored[:-1]
        assert bool((perm[1:][same] > perm[:-1][same]).all())  # stable
        assert torch.equal(torch.bincount(assignment, minlength=nlist), cell_start[1:] - cell_start[:-1])


def test_default_cell_counts():
    from muygpys_amd.neighbors import default_cells

    assert default_cells(1) == (1, 1)
    assert default_cells(10) == (3, 3)
    assert default_cells(10**6) == (1000, 16)
    assert default_cells(10**8) == (4096, 16)  # clamped: the probe selection's column limit
    assert default_cells(10**6, nlist=448) == (448, 16)
    assert default_cells(10**6, nlist=8) == (8, 8)
    assert default_cells(10**6, nlist=64, nprobe=64) == (64, 64)


def test_header_declares_the_cell_scan():
    from muygpys_amd import _abi, _lib

    assert "mgp_knn_cells_scan" in _lib.exported_names_from_header()
    restype, argtypes = _abi.signatures()["mgp_knn_cells_scan"]
    P, I, L = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    assert restype is ctypes.c_int
    # table n d | cell_start nlist | queries m | probes nprobe | self_pos | k best_d best_i | short_flag | stream
    assert argtypes == [P, L, I, P, I, P, L, P, I, P, I, P, P, P, P]


def test_cell_scan_rejects_bad_arguments_without_a_gpu():
    from muygpys_amd import _lib

    lib = _lib.load()
    buf = (ctypes.c_char * 4096)()
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) // 16 * 16)  # (a host address: no accepted call is made with it)

    def call(table=p, n=1000, d=8, cell_start=p, nlist=10, queries=p, m=5, probes=p, nprobe=3, self_pos=None, k=10,
             best_d=p, best_i=p, short_flag=p):
        return lib.mgp_knn_cells_scan(table, n, d, cell_start, nlist, queries, m, probes, nprobe, self_pos, k, best_d,
                                      best_i, short_flag, None)

    for name in ("table", "cell_start", "queries", "probes", "best_d", "best_i", "short_flag"):
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
    misaligned = ctypes.c_void_p(p.value + 4)
    assert call(table=misaligned) == _lib.EUNSUPPORTED and call(queries=misaligned) == _lib.EUNSUPPORTED
    # sizes are looked at before pointers, and an empty batch reads nothing
    assert call(table=None, k=65) == _lib.EUNSUPPORTED
    assert call(table=None, queries=None, m=0) == _lib.OK
