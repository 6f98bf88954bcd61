"""CPU: the exact grid search (NN_Wrapper(..., algorithm="grid")) without a GPU -- the numpy restatement of layout, walk
and bound (tests/knn_grid_cases.py, the yardstick of the GPU test) against fp64 brute force on every shared case, the
pure helpers of the index on CPU tensors, and the constructor's refusals."""

import numpy as np
import pytest

from tests import knn_grid_cases as G

torch = pytest.importorskip("torch")


@pytest.mark.parametrize("case", G.CASES, ids=[c.name for c in G.CASES])
def test_restatement_against_fp64_brute_force(case):
    """fp32 distances, the slack of the kernel, the stop bound: the neighbours are those of fp64 brute force (the
    project's tie rule; sorted distances on the lattice, where mass ties leave positions undefined), and the walk is
    short: the figures are printed."""
    X, Q, rows, want = G.case_data(case)
    index = G.make_index(X, case.cell_rows, case.edges)
    assert np.array_equal(np.sort(index.perm), np.arange(case.n)) and index.cell_start[-1] == case.n
    got, dist, shells, scanned = G.search(index, Q, case.k, rows)
    print(f"{case.name}: grid {index.dims}, shells mean {shells.mean():.2f} max {shells.max()}, "
          f"rows scanned per query mean {scanned.mean():.0f} max {scanned.max()}")
    if case.kind == "lattice":
        G.assert_same_distances(Q, X, got, want, case.name)
    else:
        G.assert_same_neighbours(Q, X, got, want, case.d, case.name)
    if rows is not None:
        assert not (got == rows[:, None]).any()
    assert (dist[:, 1:] >= dist[:, :-1]).all()
    assert shells.max() <= max(index.dims) - 1
    if case.kind in ("uniform", "mixture", "lattice"):  # a few hundred pair distances, not n
        assert shells.max() <= 2 and scanned.mean() < 0.1 * case.n


def test_restated_walk_widens_where_it_must():
    """Two clusters far apart and a query between them; k beyond the 3^d block; k = n - 1 (every other row)."""
    rng = np.random.default_rng(1)
    half = (rng.integers(0, 2**20, (400, 2)) / 2.0**24).astype(G.F)  # [0, 1/16)^2 and its mirror image in [15/16, 1]^2
    X = G.mirrored(half, 1.0, None, rng)
    index = G.make_index(X, 8)
    Q = np.array([[0.5, 0.375], [0.25, 0.75]], dtype=G.F)  # (off the centre of symmetry: no mirrored ties)
    got, _, shells, _ = G.search(index, Q, 10)
    G.assert_same_neighbours(Q, X, got, G.exact_neighbours(Q, X, 10), 2)
    assert shells.min() >= 3
    X = G.mirrored(rng.random((32, 3), dtype=G.F), 1.0, 0.5, rng)  # n = 65, k = 64 with self-exclusion
    index = G.make_index(X, 2)
    rows = np.arange(65)
    got, _, shells, _ = G.search(index, X, 64, rows)
    assert all(sorted(got[r].tolist()) == sorted(set(range(65)) - {r}) for r in rows)
    cells = G.cells_of(index.x, index.edges)[np.argsort(index.perm)]
    reach = np.max([np.maximum(cells[:, a], index.dims[a] - 1 - cells[:, a]) for a in range(3)], axis=0)
    assert np.array_equal(shells, reach)  # the grid's edge, whatever the data hold


def test_grid_dims():
    from muygpys_amd.neighbors import GRID_MAX_CELLS, grid_dims

    assert grid_dims(20000, [1.0, 1.0], 32) == (25, 25, 1)
    assert grid_dims(20000, [1.0, 1.0, 1.0], 16) == (11, 11, 11)
    assert grid_dims(20000, [1.0], 32) == (625, 1, 1)
    assert grid_dims(20000, [1.0, 4.0], 32) == (12, 50, 1)          # proportional to the extent
    assert grid_dims(20000, [1.0, 0.0, 2.0], 32) == (18, 1, 35)     # a zero-extent axis gets one cell
    assert grid_dims(20000, [0.0, 0.0], 32) == (1, 1, 1)
    assert grid_dims(20000, [1.0, float("nan")], 32) == (625, 1, 1)
    assert grid_dims(1000, [1.0, 1e-6], 32) == (31, 1, 1)           # thinner than a cell: the other axis takes the cells
    assert grid_dims(10, [1.0, 1.0], 32) == (1, 1, 1)
    for n, ext in ((10**9, [1.0]), (10**10, [1.0, 1.0, 1.0]), (10**12, [1.0, 3.0]), (10**10, [1.0, 1.0 + 1e-9, 1.0])):
        g = grid_dims(n, ext, 32)
        assert min(g) >= 1 and g[0] * g[1] * g[2] <= GRID_MAX_CELLS, (n, ext, g)  # capped: beyond that the cells grow
        assert g[0] * g[1] * g[2] >= 0.9 * GRID_MAX_CELLS
    with pytest.raises(ValueError, match="1 <= d <= 3"):
        grid_dims(100, [1.0] * 4)


def test_grid_cells_and_layout_invariants():
    from muygpys_amd.neighbors import cell_layout, grid_cells, grid_linear

    edges = [torch.tensor([-1.0, 0.0, 0.0, 2.5]), torch.tensor([0.5]), None]  # (equal edges: cell 2 of axis 0 is empty)
    x = torch.tensor([[-5.0, 0.0, 0], [-1.0, 0.5, 0], [-0.5, 0.4999, 0], [0.0, 9.0, 0], [2.4999, -9.0, 0], [2.5, 0.5, 0],
                      [float("inf"), float("-inf"), 0]])
    cells = grid_cells(x, edges)
    assert cells.dtype == torch.int32 and cells.shape == (7, 3)
    # a row at an edge value goes to the upper cell; the outer cells are unbounded; an axis without edges is one cell
    assert cells.tolist() == [[0, 0, 0], [1, 1, 0], [1, 0, 0], [3, 1, 0], [3, 0, 0], [4, 1, 0], [4, 0, 0]]
    dims = (5, 2, 1)
    lin = grid_linear(cells, dims)
    assert lin.dtype == torch.int64 and lin.tolist() == [0, 6, 1, 8, 3, 9, 4]  # axis 0 runs fastest
    perm, inv, cell_start = cell_layout(lin, 10)
    assert cell_start.shape == (11,) and cell_start[0] == 0 and cell_start[-1] == 7
    assert torch.equal(perm.sort().values, torch.arange(7))  # every row in exactly one cell
    stored = lin[perm]
    assert bool((stored[1:] >= stored[:-1]).all())            # cells are contiguous
    for j in range(10):
        assert bool((stored[cell_start[j]:cell_start[j + 1]] == j).all())
    # against the restatement on a random table
    rng = np.random.default_rng(2)
    X = rng.normal(size=(5000, 3)).astype(np.float32)
    index = G.make_index(X, 16)
    x4 = np.zeros((5000, 4), np.float32)
    x4[:, :3] = X - index.mean
    mine = grid_cells(torch.from_numpy(x4), [torch.from_numpy(e) for e in index.edges])
    assert np.array_equal(mine.numpy(), G.cells_of(x4, index.edges))
    p, _, cs = cell_layout(grid_linear(mine, index.dims), int(np.prod(index.dims)))
    assert np.array_equal(p.numpy(), index.perm) and np.array_equal(cs.numpy(), index.cell_start)
    assert len(cs) == int(np.prod(index.dims)) + 1


def test_constructor_refusals_name_the_limit():
    """Before anything touches a device: the limits of the route as ValueErrors, never another algorithm."""
    from muygpys_amd.neighbors import NN_Wrapper

    X = torch.randn(500, 2)
    with pytest.raises(ValueError, match="fp32"):
        NN_Wrapper(X.double(), 10, algorithm="grid")
    with pytest.raises(ValueError, match="1 <= d <= 3"):
        NN_Wrapper(torch.randn(500, 4), 10, algorithm="grid")
    with pytest.raises(ValueError, match="k <= 64"):
        NN_Wrapper(X, 65, algorithm="grid")
    with pytest.raises(ValueError, match="k <= 64"):
        NN_Wrapper(X, 0, algorithm="grid")
    with pytest.raises(ValueError, match="sorted"):
        NN_Wrapper(X, 10, algorithm="grid", edges=[torch.tensor([0.0, 1.0]), torch.tensor([1.0, 0.5])])
    with pytest.raises(ValueError, match="one edge tensor per feature"):
        NN_Wrapper(X, 10, algorithm="grid", edges=[torch.tensor([0.0])])
    with pytest.raises(ValueError, match="edges="):
        NN_Wrapper(X, 10, algorithm="grid", edges="kmeans")
    with pytest.raises(ValueError, match="cell_rows"):
        NN_Wrapper(X, 10, algorithm="grid", cell_rows=0)
    # within the limits the next thing asked for is the device; any other value of the keyword is ignored as before
    for kwargs in (dict(algorithm="grid"), dict(algorithm="kd_tree"), dict()):
        with pytest.raises(TypeError, match="ROCm device"):
            NN_Wrapper(X, 10, **kwargs)
    with pytest.raises(TypeError, match="ROCm device"):
        NN_Wrapper(X.double(), 10, algorithm="ball_tree")
