"""k-nearest-neighbour index producer on the GPU: exact brute force, or an inverted-cell index.

The step immediately upstream of the hot path: the reference wraps scikit-learn's exact KNN
(or hnswlib) on the CPU (src/MuyGPyS/neighbors.py:32-262).  ``NN_Wrapper`` here keeps that
interface -- ``get_nns(test)`` / ``get_batch_nns(batch_indices)`` returning ``(indices int64,
squared-l2 distances)`` with the self-match dropped for batch queries (neighbors.py:207-211,
246-250) -- and computes it exactly.

* fp32, ``d <= 64``, ``k <= 64`` (the shapes of the hot path): the fused MFMA
  scan ``mgp_knn_scan_f32`` (``csrc/mgp_knn.hip``) -- distances on the matrix cores, one compare
  per pair against the query's running k-th best, rare survivors merged into per-query k-best
  lists -- after the lists have been initialised from the first rows of the table on the dense
  path.  Nothing of size (queries x train) is ever materialised.  The kernels take rows of a multiple of four
  features: the table is stored zero-padded to ``_width`` = max(4, 4 ceil(d / 4)) after centring and the queries are
  padded alike (distances do not change; ``feature_count`` stays the caller's d) -- d = 1, 2, 3 (spatial tables), 5, 10,
  30 ... run on the scans too; ``MUYGPYS_HIP_KNN_PAD=0`` keeps them on the dense path.
* the same tables, ``64 < k <= 1024``: the wide-list scan ``mgp_knn_scan_wide`` and its finish step
  ``mgp_knn_finish_wide`` (``csrc/mgp_knn_wide.hip``) -- the same arithmetic, the lists in global memory and held by
  the draining wave as ceil(k / 64) entries per lane, a queue slot per column of the tile, so no queue can overflow;
  the lists start from ``SCAN_INIT_ROWS`` head rows.  3 to 24 times the dense path at 1 M x 1 M
  (``profiles/knn_wide_bench.json``); ``MUYGPYS_HIP_KNN_WIDE=0`` keeps these searches on the dense path.
* fp32, ``64 < d <= 256`` (the reference torch tutorial's 100-dimensional embedding), ``k <= 1024``: the long-row scans
  ``mgp_knn_scan_long`` (k <= 64) / ``mgp_knn_scan_long_wide`` (``csrc/mgp_knn_long.hip``) -- the same arithmetic,
  a 64-row tile staged in ceil(d / 64) feature chunks with the accumulators carried across them -- from
  ``SCAN_INIT_ROWS`` head rows, then the same finish entries.  4 to 10 times the dense path at 1 M x 1 M
  (``profiles/knn_long_bench.json``); ``MUYGPYS_HIP_KNN_LONG=0`` keeps these searches on the dense path.
* anything else (fp64 tables, tables of up to 8 192 rows, ``use_scan=False``, d > 256): the dense path, in row chunks,
  ``|q|^2 + |x|^2 - 2 q.x`` through ``torch.matmul`` (rocBLAS) followed by ``topk``.

``scan_route(d, k, dtype, train_count, use_scan)`` is the rule, a pure function; ``last_route`` ("scan" | "wide" |
"long" | "dense" | "ivf" | "grid") names what served the most recent search.

Either way the k winners are then re-measured in difference form and sorted, so the returned
distances carry no cancellation error and ties resolve by distance then index order of the sort.

``nn_method="ivf"`` is the approximate search (the role of the reference's ``nn_method="hnsw"``,
neighbors.py:109-127,213-262; a graph walk suits a GPU badly): k-means cells over the table, the table stored
cell by cell, and every query scans only its ``nprobe`` nearest cells (``mgp_knn_cells_scan``,
``csrc/mgp_knn_cells.hip``).  fp32 only, ``d <= 64``, ``k <= 64``; the neighbours are exact within the probed
cells and approximate over the table -- good on data with low-dimensional structure (clusters, manifolds), poor on
data without (i.i.d. Gaussian at d = 40: recall 0.49 at 8 of 64 cells in a CPU simulation).  A query whose probed
cells hold fewer than k rows is recomputed exactly on the dense path.

``nn_method="exact", algorithm="grid"`` is the exact search for tables of 1 to 3 features (the role of the reference's
``algorithm="kd_tree"`` / ``"ball_tree"``, which it hands to scikit-learn; every other value of ``algorithm`` is
ignored, and the default route does not change).  The centred table is stored cell by cell over a rectilinear grid
(``grid_dims``: near-cubic cells of ``cell_rows`` rows on average; ``edges="uniform"`` | ``"quantile"`` | a list of d
edge tensors; cells are defined by comparisons against the stored edges, ``grid_cells``), and every query walks the
cells around its own shell by shell until the distance to the faces of the walked block proves its list final
(``mgp_knn_grid_scan``, ``csrc/mgp_knn_grid.hip``): a few hundred pair distances per query instead of n.  fp32 only,
``1 <= d <= 3``, ``k <= 64``, ``n < 2^31``: anything else is a ``ValueError`` at construction, never another algorithm.
``last_route`` is "grid" and ``last_shells`` holds, per query, the radius in cells of the last shell walked.  A query
with a NaN feature is at no distance from anything (and so is every query of a table that holds a NaN: the mean it is
centred on is NaN): its walk ends at the grid's edge with an empty list, it is flagged in ``last_short`` (device int32,
1 per query left with fewer than k neighbours), and its entries name the row at stored position 0 (``_perm[0]``) at a
NaN distance.  ``cell_rows`` defaults to 16, the best of the sweep of ``tools/knngridbench.py`` at 1 M rows
(``profiles/knn_grid_bench.json``).
"""

from __future__ import annotations

import os

import math

from typing import Tuple

import torch

from . import _lib

SCAN_INIT_ROWS = 4096  # rows of the table the k-best lists are initialised from (dense path)
WIDE_MAX_K = 1024      # mgp_knn_wide_max_nn_count(): the longest list of the wide scan (64 < k: csrc/mgp_knn_wide.hip)
LONG_MAX_D = 256       # mgp_knn_long_max_features(): the widest row of the long-row scans (64 < d: csrc/mgp_knn_long.hip)
CELLS_MAX = 4096       # most cells of the inverted-cell index: mgp_topk_rows_f32's column limit (probe selection)
CELLS_SAMPLE = 256     # k-means runs on at most this many rows per cell
GRID_MAX_D = 3         # most features of the grid walk (3^d cells around a query: csrc/mgp_knn_grid.hip)
GRID_MAX_CELLS = 1 << 24  # most cells of a grid (mgp_knn_grid_scan's limit): beyond that the cells grow
GRID_CELL_ROWS = 16    # mean rows per cell of a grid where the caller names none: the sweep's best at 1 M rows


def stored_width(d: int) -> int:
    """The row width the scan kernels see: the next multiple of four, four at least (rows are zero-padded to it)."""
    return max(4, -(-int(d) // 4) * 4)


def _switch(name: str) -> bool:
    return os.environ.get(name, "1") != "0"  # (read on every call: A/B on a live object)


def scan_route(d: int, k: int, dtype, train_count: int, use_scan: bool = True):
    """Which kernels serve an exact search of ``k`` neighbours in a ``dtype`` table of ``train_count`` rows of ``d``
    features: "scan" (k <= 64) or "wide" (k <= 1024) at a stored width of up to 64, "long" at 68 to 256, None for the
    dense path.  A pure function of its arguments and the three A/B switches of the environment
    (MUYGPYS_HIP_KNN_WIDE / _LONG / _PAD = 0: k > 64 / stored widths > 64 / padded widths stay dense)."""
    if not use_scan or dtype != torch.float32 or d < 1 or k < 1:
        return None
    if not 2 * SCAN_INIT_ROWS < train_count < 2**31:
        return None
    width = stored_width(d)
    if width != d and not _switch("MUYGPYS_HIP_KNN_PAD"):
        return None
    if k > (WIDE_MAX_K if _switch("MUYGPYS_HIP_KNN_WIDE") else 64):
        return None
    if width <= 64:
        return "wide" if k > 64 else "scan"
    if width <= LONG_MAX_D and _switch("MUYGPYS_HIP_KNN_LONG"):
        return "long"
    return None


def default_cells(train_count: int, nlist=None, nprobe=None) -> Tuple[int, int]:
    """(nlist, nprobe) of the inverted-cell index where the caller names none: round(sqrt(n)) cells, clamped to
    [1, CELLS_MAX], and min(nlist, 16) probed cells."""
    if nlist is None:
        nlist = min(CELLS_MAX, max(1, int(round(math.sqrt(train_count)))))
    if nprobe is None:
        nprobe = min(int(nlist), 16)
    return int(nlist), int(nprobe)


def cell_layout(assignment: torch.Tensor, nlist: int):
    """The storage order of an assignment vector (row -> cell): ``perm`` (stored position -> row; a stable sort by
    cell, so rows keep their order within a cell), ``inv`` (row -> stored position) and ``cell_start`` (int64,
    nlist + 1: cell j is stored at [cell_start[j], cell_start[j + 1]); empty cells are legal).  Any device."""
    assignment = assignment.to(torch.int64)
    perm = torch.argsort(assignment, stable=True)
    inv = torch.empty_like(perm)
    inv[perm] = torch.arange(perm.numel(), device=perm.device)
    cell_start = torch.zeros(nlist + 1, dtype=torch.int64, device=assignment.device)
    cell_start[1:] = torch.bincount(assignment, minlength=nlist).cumsum(0)
    return perm, inv, cell_start


def grid_dims(n: int, extents, cell_rows: float = GRID_CELL_ROWS) -> Tuple[int, int, int]:
    """(g0, g1, g2) of the grid over a table of ``n`` rows whose axes span ``extents`` (one to three numbers): near-cubic
    cells, g_a proportional to the axis extent, g0 g1 g2 ~ n / cell_rows and at most GRID_MAX_CELLS (beyond that the
    cells grow).  g_a = 1 on an axis the table does not have, on an axis of zero (or non-finite) extent and on an axis
    thinner than one cell.  A pure function."""
    ext = [float(v) for v in extents]
    if not 1 <= len(ext) <= GRID_MAX_D:
        raise ValueError(f"a grid has 1 to {GRID_MAX_D} axes (1 <= d <= {GRID_MAX_D}), got {len(ext)}")
    target = min(GRID_MAX_CELLS, max(1, int(round(n / float(cell_rows)))))
    g = [1, 1, 1]
    active = [a for a, v in enumerate(ext) if v > 0 and math.isfinite(v)]
    side = 0.0
    while active:
        side = math.exp((sum(math.log(ext[a]) for a in active) - math.log(target)) / len(active))
        thin = [a for a in active if ext[a] < side]  # (not one cell wide: one cell, and the others share the target)
        if not thin:
            break
        active = [a for a in active if a not in thin]
    for a in active:
        g[a] = max(1, int(round(ext[a] / side)))
    while g[0] * g[1] * g[2] > GRID_MAX_CELLS:  # (rounding up on every axis at the cap)
        g[g.index(max(g))] -= 1
    return g[0], g[1], g[2]


def grid_cells(x: torch.Tensor, edges) -> torch.Tensor:
    """(m, 3) int32: the cell of every row of ``x`` (m, >= d) per axis, c_a = #{j : E_a[j] <= x_a} against the interior
    edges ``edges[a]`` (1-D, non-decreasing; an axis without edges is one cell).  Comparisons against the stored edge
    values, never a division: a row at an edge value goes to the upper cell.  Any device."""
    out = torch.zeros((x.shape[0], 3), dtype=torch.int32, device=x.device)
    for a, e in enumerate(edges):
        if e is not None and e.numel():
            out[:, a] = torch.bucketize(x[:, a].contiguous(), e, right=True).to(torch.int32)
    return out


def grid_linear(cells: torch.Tensor, dims) -> torch.Tensor:
    """The linear cell id (int64) of per-axis cells (m, 3): axis 0 runs fastest."""
    c = cells.to(torch.int64)
    return c[:, 0] + dims[0] * (c[:, 1] + dims[1] * c[:, 2])


class NN_Wrapper:
    def __init__(self, train: torch.Tensor, nn_count: int, nn_method: str = "exact", chunk: int = 4096,
                 use_scan: bool = True, scan_kind: str = "auto", shuffle: bool = True, nlist=None, nprobe=None,
                 kmeans_iters: int = 10, seed: int = 0, _cells=None, algorithm=None, edges="uniform",
                 cell_rows=GRID_CELL_ROWS, **kwargs):
        if nn_method.lower() not in ("exact", "ivf"):
            raise NotImplementedError(f"Nearest Neighbor algorithm {nn_method} is not implemented.")
        self.algorithm = None  # "grid": the grid walk serves every search (any other value of the keyword is ignored)
        grid = nn_method.lower() == "exact" and algorithm == "grid" and isinstance(train, torch.Tensor)
        if grid:  # (its limits before anything else: they need no device)
            self._check_grid(train, nn_count, edges, cell_rows)
        if not (isinstance(train, torch.Tensor) and train.is_cuda):
            raise TypeError("NN_Wrapper takes a torch tensor on the ROCm device")
        if nn_method.lower() == "ivf":
            self._init_cells(train, nn_count, nlist, nprobe, kmeans_iters, seed, chunk, _cells)
            return
        if grid:
            self._init_grid(train, nn_count, edges, cell_rows, chunk)
            return
        # the table is kept centred on its mean (queries are shifted alike): distances are unchanged,
        # and every Gram-form quantity below (|q|^2 + |x|^2 - 2 q.x, the split-bf16 margin) is computed
        # at the scale of the data's spread instead of its offset from the origin
        table = train[:, None] if train.ndim == 1 else train
        self._mean = table.double().mean(0).to(table.dtype)
        self.train_count, self.feature_count = table.shape
        # Tables the scan kernels serve are also stored in a fixed pseudo-random row order: a table
        # sorted in space (a grid, a time series) would hand a query all of its neighbours within one or
        # two consecutive tiles and overflow the kernels' candidate queues; shuffled, candidates arrive
        # evenly and the first rows are a fair sample for the initial k-best lists.  ``_perm`` maps
        # stored position -> caller's row, ``_inv`` the other way; both are None for the identity.
        self._perm = self._inv = None
        # ... and with their rows zero-padded to the width the kernels take (a multiple of four, four at least; the
        # queries are padded alike, after centring: distances do not change).  ``feature_count`` stays the caller's.
        # (k = 1 and every switch on: could a scan ever serve this table?)
        served = (use_scan and table.dtype == torch.float32 and 2 * SCAN_INIT_ROWS < self.train_count < 2**31
                  and stored_width(self.feature_count) <= LONG_MAX_D)
        self._width = stored_width(self.feature_count) if served else self.feature_count
        table = self._pad_features(table - self._mean)
        if shuffle and served:
            gen = torch.Generator(device=table.device).manual_seed(0x5CA9)
            self._perm = torch.randperm(self.train_count, device=table.device, generator=gen)
            self._inv = torch.empty_like(self._perm)
            self._inv[self._perm] = torch.arange(self.train_count, device=table.device)
            self.train = table[self._perm].contiguous()
        else:
            self.train = table
        self.nn_count = int(nn_count)
        self.nn_method = "exact"
        self.chunk = int(chunk)
        self.use_scan = bool(use_scan)
        if scan_kind not in ("auto", "bf16x3", "f32"):
            raise ValueError("scan_kind must be 'auto', 'bf16x3' or 'f32'")
        # measured (1 M x 1 M, end to end): split-bf16 pre-filter 0.47 s (d = 40) / 0.36 s (d = 8),
        # plain fp32 scan 0.90 s / 0.43 s
        self.scan_kind = "bf16x3" if scan_kind == "auto" else scan_kind
        self._packed_train, self._packed_qmax, self._packed_layout = None, None, None
        self.last_overflow = None  # per-query overflow flags of the most recent scan (device int32)
        self.last_route = None     # what served the most recent search: "scan" | "wide" | "long" | "dense" | "ivf"
        self._sq = (self.train.double() ** 2).sum(1).to(self.train.dtype)
        # the scan kernel reads |x|^2 in whole 64-row tiles: +inf past the end (never a neighbour)
        pad = (-self.train_count) % 64
        self._sq_scan = torch.cat([self._sq, torch.full((pad,), float("inf"), device=self._sq.device, dtype=self._sq.dtype)])

    def get_nns(self, test: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """neighbors.py:129-167: nn_count nearest training rows of every test row."""
        test = test[:, None] if test.ndim == 1 else test
        return self._get_nns(test, self.nn_count)

    def get_batch_nns(self, batch_indices: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """neighbors.py:169-211: neighbours of training rows, the row itself excluded.  (The
        reference drops column 0 of a k+1 query and relies on it being the point itself; here the
        self-match is masked explicitly, so duplicate points cannot displace it.)"""
        pos = batch_indices if self._inv is None else self._inv[batch_indices]
        return self._get_nns(self.train[pos], self.nn_count, exclude=pos, centred=True)

    def _get_nns(self, samples, nn_count, exclude=None, centred=False):
        if not centred:
            samples = samples.to(self.train.dtype) - self._mean
        if self.nn_method == "ivf":
            self.last_route = "ivf"
            return self._cells_nns(samples, nn_count, exclude)
        if self.algorithm == "grid":
            self.last_route = "grid"
            return self._grid_nns(samples, nn_count, exclude)
        samples = self._pad_features(samples)
        out = self._scan_nns(samples, nn_count, exclude)  # (sets last_route where it serves the call)
        if out is None:
            self.last_route = "dense"
            out = self._dense_nns(samples, nn_count, exclude)
        idx, dist = out
        return (idx if self._perm is None else self._perm[idx]), dist

    def _route(self, samples, nn_count):
        """scan_route for this table and these (centred, padded) query rows."""
        if samples.dtype != self.train.dtype or samples.shape[1] != self._width or self._width % 4:
            return None
        return scan_route(self.feature_count, int(nn_count), self.train.dtype, self.train_count, self.use_scan)

    def _scan_supported(self, samples, nn_count) -> bool:
        return self._route(samples, nn_count) is not None

    @staticmethod
    def _split_bf16(v: torch.Tensor):
        hi = v.to(torch.bfloat16)
        return hi, (v - hi.float()).to(torch.bfloat16)

    @classmethod
    def _pack_bf16(cls, x: torch.Tensor, slot_a, slot_b) -> torch.Tensor:
        """Rows [hi(KP) | lo(KP)] of the split x = hi + lo (bf16 each), KP = 16 ceil((d + 2) / 16); the
        last two slots of each part hold the split of ``slot_a`` / ``slot_b`` (scalars or (n,) tensors):
        the threshold terms the scan kernel evaluates on the matrix cores (csrc/mgp_knn.hip)."""
        n, d = x.shape
        kp = (d + 2 + 15) // 16 * 16
        packed = torch.zeros((n, 2 * kp), device=x.device, dtype=torch.bfloat16)
        packed[:, :d], packed[:, kp:kp + d] = cls._split_bf16(x)
        for pos, val in ((kp - 2, slot_a), (kp - 1, slot_b)):
            val = torch.as_tensor(val, device=x.device, dtype=torch.float32).expand(n)
            packed[:, pos], packed[:, kp + pos] = cls._split_bf16(val)
        return packed

    @classmethod
    def _pack_bf16_d8(cls, x: torch.Tensor, slot_a, slot_b) -> torch.Tensor:
        """d <= 8 (mgp_knn_scan_bf16x2_d8): rows [hi(8) | lo(8) | T(8)].  The threshold terms are one product of the T
        parts: a table row (``slot_a`` = c, ``slot_b`` = 1) carries T = [hi(c), lo(c), 1, 1, 0 ...], a query row
        (``slot_a`` = 1, ``slot_b`` = 0) T = [1, 1, 0, 0, 0 ...] -- the kernel writes the split of -thr into slots 2, 3."""
        n, d = x.shape
        packed = torch.zeros((n, 24), device=x.device, dtype=torch.bfloat16)
        packed[:, :d], packed[:, 8:8 + d] = cls._split_bf16(x)
        if torch.is_tensor(slot_a):  # table rows
            packed[:, 16], packed[:, 17] = cls._split_bf16(slot_a.to(torch.float32))
            packed[:, 18:20] = 1.0
        else:  # query rows
            packed[:, 16:18] = 1.0
        return packed

    def _scan_nns(self, samples, nn_count, exclude=None, force_wide=False):
        """Fused MFMA scan (see the module docstring); None when the shape is not covered.  ``force_wide``: the wide
        pair for k <= 64 too (tools/knnwidebench.py's sanity line; no search is routed that way)."""
        route = self._route(samples, nn_count)
        if route is None:
            return None
        q = samples.contiguous()
        m, k = q.shape[0], int(nn_count)
        if m == 0:
            return None
        # exact k-best over the first rows of the table (Gram-form distances, like the scan's).  How many rows: a query
        # collects ~ k / rows-seen candidates per row and its queue (16 entries) is emptied once per tile at the
        # earliest, so the first tile -- 128 rows for the short packed rows, 64 otherwise -- should bring two at most
        # (P(Poisson(2) >= 17) ~ 5e-11): tile * k / 2 rows, in steps of 1 024, SCAN_INIT_ROWS at most.  torch's topk
        # over these rows was a fifth of the search's time at 1 M x 1 M, k = 30 (round 5)
        # Lists of more than 64 entries (mgp_knn_scan_wide): its queues cannot overflow whatever the head rows are, and
        # the more rows the lists start from the fewer candidates the scan merges: SCAN_INIT_ROWS for every k
        # Long rows (mgp_knn_scan_long): SCAN_INIT_ROWS too -- its 16-entry queues then see 64 k / 4096 <= 1 expected
        # survivor per tile
        wide = k > 64 or force_wide
        long_rows = route == "long"
        tile_rows = 128 if (self.scan_kind == "bf16x3" and self._width + 2 <= 16) else 64
        init_rows = SCAN_INIT_ROWS if wide or long_rows else min(SCAN_INIT_ROWS, max(1024, -(-(tile_rows * k // 2) // 1024) * 1024))
        head = self.train[:init_rows]
        best_d = torch.empty((m, k), device=q.device, dtype=torch.float32)
        best_i = torch.empty((m, k), device=q.device, dtype=torch.int32)
        qn = (q * q).sum(1)
        init_chunk = max(self.chunk, 16384)  # (a 16 384 x 4 096 distance block is 268 MB; fewer, larger launches)
        for s in range(0, m, init_chunk):
            qq = q[s:s + init_chunk]
            d2 = self._sq[None, :init_rows] - 2.0 * (qq @ head.T) + qn[s:s + init_chunk, None]
            if exclude is not None:
                ex = exclude[s:s + init_chunk]
                inside = ex < init_rows
                rows = torch.arange(qq.shape[0], device=q.device)[inside]
                d2[rows, ex[inside]] = float("inf")
            # the k smallest per row, unordered (csrc/mgp_knn_select.hip: one wave per row, bisection on the key bits);
            # torch.topk's multi-block radix select on a million short rows was a sixth of the search (round 5)
            rc_sel = _lib.load().mgp_topk_rows_f32(_lib.ptr(d2), d2.shape[0], d2.shape[1], d2.stride(0), k,
                                                   _lib.ptr(best_d[s:s + init_chunk]), _lib.ptr(best_i[s:s + init_chunk]),
                                                   _lib.stream_ptr())
            if rc_sel == _lib.EUNSUPPORTED:  # (more than 4 096 columns: not this path's sizes)
                bd, bi = d2.topk(k, dim=1, largest=False)
                best_d[s:s + init_chunk] = bd
                best_i[s:s + init_chunk] = bi.to(torch.int32)
            else:
                _lib.check(rc_sel, "mgp_topk_rows_f32")
        overflow = torch.zeros((m,), device=q.device, dtype=torch.int32)
        ex64 = None if exclude is None else exclude.to(torch.int64).contiguous()
        if wide:
            return self._wide_nns(q, qn, ex64, exclude, init_rows, best_d, best_i, overflow, long_rows)
        if self.scan_kind == "bf16x3" and not long_rows:  # (the long rows have no split-bf16 pre-filter)
            # the split-bf16 kernel keeps exact (difference-form) distances in the lists
            for s in range(0, m, 65536):
                diff = q[s:s + 65536, None, :] - self.train[best_i[s:s + 65536].to(torch.int64)]
                best_d[s:s + 65536] = (diff * diff).sum(-1)
            # table rows carry c = -|x|^2/2 + 2^-14 QMAX |x| (raised by its own split error) and a 1;
            # query rows a 1 and a slot the kernel fills with -(|q|^2 - tau)/2
            # QMAX only has to bound |q| from above (a larger margin lets a few more near misses
            # through to the exact re-measurement): the packed table is rebuilt only when a batch
            # exceeds the bound it was packed for, with head-room so that it rarely does
            qmax = float(qn.max().sqrt())
            # d <= 8: the two-chain kernel on 24-slot rows (round 5), else three chains on [hi(KP) | lo(KP)]
            d8 = self._width <= 8 and os.environ.get("MUYGPYS_HIP_KNN_D8", "1") != "0"  # (0: A/B against the three-chain kernel)
            pack = self._pack_bf16_d8 if d8 else self._pack_bf16
            scan = _lib.load().mgp_knn_scan_bf16x2_d8 if d8 else _lib.load().mgp_knn_scan_bf16x3
            # (the cache remembers WHICH layout it holds: the A/B switch may be flipped on a live object)
            if self._packed_train is None or self._packed_layout != d8 or qmax > self._packed_qmax:
                self._packed_layout = d8
                self._packed_qmax = 1.25 * qmax
                c = -0.5 * self._sq + (2.0**-14 * self._packed_qmax) * self._sq.sqrt()
                c = c + 2.0**-15 * c.abs()
                self._packed_train = pack(self.train, c, 1.0)
            packed_q = pack(q, 1.0, 0.0)
            rc = scan(
                _lib.ptr(self.train), _lib.ptr(self._packed_train), _lib.ptr(self._sq_scan), self.train_count,
                self._width, _lib.ptr(q), _lib.ptr(packed_q), _lib.ptr(qn), _lib.ptr(ex64), m, k,
                init_rows, _lib.ptr(best_d), _lib.ptr(best_i), _lib.ptr(overflow), _lib.stream_ptr(),
            )
        else:
            scan = _lib.load().mgp_knn_scan_long if long_rows else _lib.load().mgp_knn_scan_f32
            rc = scan(
                _lib.ptr(self.train), _lib.ptr(self._sq_scan), self.train_count, self._width,
                _lib.ptr(q), _lib.ptr(qn), _lib.ptr(ex64), m, k, init_rows,
                _lib.ptr(best_d), _lib.ptr(best_i), _lib.ptr(overflow), _lib.stream_ptr(),
            )
        if rc == _lib.EUNSUPPORTED:  # MGP_EUNSUPPORTED (alignment)
            return None
        _lib.check(rc, "mgp_knn_scan_f32")
        # the winners re-measured in difference form, put in order and mapped to the caller's row numbers in one launch
        # (csrc/mgp_knn_select.hip) -- was gather (m, k, d) / subtract / square / sum / argsort / gather / gather
        idx = torch.empty((m, k), dtype=torch.int64, device=q.device)
        dist = torch.empty((m, k), dtype=q.dtype, device=q.device)
        rc_fin = _lib.load().mgp_knn_finish_f32(_lib.ptr(q), _lib.ptr(self.train), self._width, _lib.ptr(best_i), m, k,
                                                None, _lib.ptr(idx), _lib.ptr(dist), _lib.stream_ptr())
        if rc_fin == _lib.EUNSUPPORTED:
            cand = best_i.to(torch.int64)
            for s in range(0, m, 65536):
                c = cand[s:s + 65536]
                diff = q[s:s + 65536, None, :] - self.train[c]
                dd = (diff * diff).sum(-1)
                order = dd.argsort(dim=1, stable=True)
                idx[s:s + 65536] = c.gather(1, order)
                dist[s:s + 65536] = dd.gather(1, order)
        else:
            _lib.check(rc_fin, "mgp_knn_finish_f32")
        self.last_overflow = overflow
        redo = overflow.nonzero().reshape(-1)
        if redo.numel():  # queues overflowed (adversarial row order): those queries go dense
            ri, rd = self._dense_nns(q[redo], k, None if exclude is None else exclude[redo])
            idx[redo], dist[redo] = ri, rd
        self.last_route = route
        return idx, dist

    FINISH_BUDGET_BYTES = 1 << 30  # the (rows, k, d) temporary of the torch finish step, where the kernel declines

    def _wide_nns(self, q, qn, ex64, exclude, init_rows, best_d, best_i, overflow, long_rows=False):
        """The scan and the finish step for 64 < k <= WIDE_MAX_K (csrc/mgp_knn_wide.hip; ``long_rows``: stored widths
        beyond 64, csrc/mgp_knn_long.hip) on lists that hold the exact k-best of the first ``init_rows`` rows (Gram
        form); None where the scan declines (alignment)."""
        (m, k), d = best_d.shape, self._width
        scan = _lib.load().mgp_knn_scan_long_wide if long_rows else _lib.load().mgp_knn_scan_wide
        rc = scan(
            _lib.ptr(self.train), _lib.ptr(self._sq_scan), self.train_count, d, _lib.ptr(q), _lib.ptr(qn),
            _lib.ptr(ex64), m, k, init_rows, _lib.ptr(best_d), _lib.ptr(best_i), _lib.ptr(overflow), _lib.stream_ptr(),
        )
        if rc == _lib.EUNSUPPORTED:
            return None
        _lib.check(rc, "mgp_knn_scan_wide")
        idx = torch.empty((m, k), dtype=torch.int64, device=q.device)
        dist = torch.empty((m, k), dtype=q.dtype, device=q.device)
        rc_fin = _lib.load().mgp_knn_finish_wide(_lib.ptr(q), _lib.ptr(self.train), d, _lib.ptr(best_i), m, k,
                                                 None, _lib.ptr(idx), _lib.ptr(dist), _lib.stream_ptr())
        if rc_fin == _lib.EUNSUPPORTED:
            # rows per pass from a byte budget: the gathered (rows, k, d) block and its squares (at k = 1023, d = 40 a
            # fixed 65 536 rows would be 10.7 GB)
            rows = max(1, self.FINISH_BUDGET_BYTES // (2 * k * d * q.element_size()))
            for s in range(0, m, rows):
                c = best_i[s:s + rows].to(torch.int64)
                diff = q[s:s + rows, None, :] - self.train[c]
                dd = (diff * diff).sum(-1)
                order = dd.argsort(dim=1, stable=True)
                idx[s:s + rows] = c.gather(1, order)
                dist[s:s + rows] = dd.gather(1, order)
        else:
            _lib.check(rc_fin, "mgp_knn_finish_wide")
        self.last_overflow = overflow
        redo = overflow.nonzero().reshape(-1)
        if redo.numel():  # (the contract of the narrow scans; the wide scan's queues cannot overflow)
            ri, rd = self._dense_nns(q[redo], k, None if exclude is None else exclude[redo])
            idx[redo], dist[redo] = ri, rd
        self.last_route = "long" if long_rows else "wide"
        return idx, dist

    DENSE_BUDGET_BYTES = 4 << 30  # (chunk x train_count) distance matrix + topk temporaries

    def _dense_nns(self, samples, nn_count, exclude=None):
        n = samples.shape[0]
        idx = torch.empty((n, nn_count), dtype=torch.int64, device=samples.device)
        dist = torch.empty((n, nn_count), dtype=samples.dtype, device=samples.device)
        # query rows per pass from a memory budget: the distance matrix of a pass is chunk x train_count
        per_row = 3 * self.train_count * self.train.element_size()
        chunk = max(1, min(self.chunk, self.DENSE_BUDGET_BYTES // max(per_row, 1)))
        for s in range(0, n, chunk):
            q = samples[s:s + chunk].to(self.train.dtype)
            d2 = self._sq[None, :] - 2.0 * (q @ self.train.T) + (q * q).sum(1)[:, None]
            if exclude is not None:
                rows = torch.arange(q.shape[0], device=q.device)
                d2[rows, exclude[s:s + chunk]] = float("inf")
            _, cand = d2.topk(nn_count, dim=1, largest=False)
            # exact squared distances of the winners, difference form, then final order
            diff = q[:, None, :] - self.train[cand]
            dd = (diff * diff).sum(-1)
            order = dd.argsort(dim=1, stable=True)
            idx[s:s + chunk] = cand.gather(1, order)
            dist[s:s + chunk] = dd.gather(1, order)
        return idx, dist

    # ---- the inverted-cell index (nn_method="ivf") -------------------------------------------------------------------

    @classmethod
    def _from_cells(cls, train, nn_count, centroids, assignment, nprobe=None, **kwargs):
        """An index over the caller's cells: ``centroids`` (nlist, d) in the table's coordinates and ``assignment``
        (n) row -> cell, taken as they are (no k-means; a row need not sit in its nearest cell)."""
        return cls(train, nn_count, nn_method="ivf", nprobe=nprobe, _cells=(centroids, assignment), **kwargs)

    def _pad_features(self, x: torch.Tensor) -> torch.Tensor:
        """Rows zero-padded to the stored width (the next multiple of 4): distances do not change."""
        if x.shape[1] == self._width:
            return x.contiguous()
        out = torch.zeros((x.shape[0], self._width), device=x.device, dtype=x.dtype)
        out[:, :x.shape[1]] = x
        return out

    def _init_cells(self, train, nn_count, nlist, nprobe, kmeans_iters, seed, chunk, cells):
        table = train[:, None] if train.ndim == 1 else train
        n, d = table.shape
        k = int(nn_count)
        # the cell scan's contract (include/muygpys_hip.h: mgp_knn_cells_scan); no other algorithm steps in
        if table.dtype != torch.float32:
            raise ValueError(f"nn_method='ivf' serves float32 tables only (fp32 only), got {table.dtype}")
        if d > 64:
            raise ValueError(f"nn_method='ivf' serves at most 64 features (d <= 64), got d = {d}")
        if not 1 <= k <= 64:
            raise ValueError(f"nn_method='ivf' serves 1 <= nn_count <= 64 (k <= 64), got k = {k}")
        if not 1 <= n < 2**31:
            raise ValueError(f"nn_method='ivf' serves 1 <= n < 2^31 table rows, got n = {n}")
        self.train_count, self.feature_count = n, d
        self.nn_count, self.nn_method, self.chunk = k, "ivf", int(chunk)
        self.use_scan, self.scan_kind, self.last_overflow, self.last_route = False, None, None, None
        self.last_short = None  # per query: 1 where the probed cells held fewer than k rows (recomputed exactly)
        self._width = max(4, -(-d // 4) * 4)
        self._mean = table.double().mean(0).to(table.dtype)
        x = self._pad_features(table - self._mean)
        self._kmeans_init = self._kmeans_sample = None
        if cells is not None:
            centroids, assignment = cells
            nlist = int(centroids.shape[0])
            centroids = centroids[:, None] if centroids.ndim == 1 else centroids
            if centroids.shape[1] != d or assignment.shape != (n,):
                raise ValueError("_from_cells takes centroids (nlist, d) and an assignment (n)")
            centroids = self._pad_features(centroids.to(device=x.device, dtype=x.dtype) - self._mean)
            assignment = assignment.to(device=x.device, dtype=torch.int64)
            if n and not (0 <= int(assignment.min()) and int(assignment.max()) < nlist):
                raise ValueError("_from_cells: the assignment names a cell outside [0, nlist)")
        nlist, nprobe = default_cells(n, nlist, nprobe)
        most = CELLS_MAX if cells is not None else min(n, CELLS_MAX)  # (k-means starts from nlist distinct rows)
        if not 1 <= nlist <= most:
            raise ValueError(f"nn_method='ivf' serves 1 <= nlist <= min(n, {CELLS_MAX}), got nlist = {nlist}")
        if not 1 <= nprobe <= nlist:
            raise ValueError(f"nn_method='ivf' serves 1 <= nprobe <= nlist, got nprobe = {nprobe}, nlist = {nlist}")
        self.nlist, self.nprobe = nlist, nprobe
        if cells is None:
            centroids = self._kmeans(x, nlist, int(kmeans_iters), int(seed))
            assignment = self._nearest_cell(x, centroids)
        self._centroids = centroids.contiguous()
        self._csq = (self._centroids.double() ** 2).sum(1).to(x.dtype)
        self._perm, self._inv, self.cell_start = cell_layout(assignment, nlist)
        self.train = x[self._perm].contiguous()
        self._sq = (self.train.double() ** 2).sum(1).to(self.train.dtype)  # (the dense path of the short queries)

    @property
    def centroids(self) -> torch.Tensor:
        """(nlist, d) cell centres in the table's coordinates."""
        return self._centroids[:, :self.feature_count] + self._mean

    @staticmethod
    def _nearest_cell(x: torch.Tensor, centroids: torch.Tensor) -> torch.Tensor:
        """argmin_j |x - c_j|^2 per row, Gram form (|x|^2 does not move the argmin), in row chunks."""
        csq = (centroids * centroids).sum(1)
        out = torch.empty(x.shape[0], dtype=torch.int64, device=x.device)
        rows = max(1, (1 << 26) // centroids.shape[0])
        for s in range(0, x.shape[0], rows):
            out[s:s + rows] = torch.addmm(csq[None, :], x[s:s + rows], centroids.T, alpha=-2.0).argmin(1)
        return out

    def _kmeans(self, x: torch.Tensor, nlist: int, iters: int, seed: int) -> torch.Tensor:
        """``iters`` Lloyd passes from ``nlist`` distinct rows drawn by a seeded device generator, on a sample of at
        most CELLS_SAMPLE rows per cell.  An empty cell keeps its centroid.  The sums go through index_put_ with
        accumulate (a sort by cell, one order of addition) instead of index_add_'s atomics: the same seed gives
        the same index bit for bit."""
        n = x.shape[0]
        gen = torch.Generator(device=x.device).manual_seed(seed)
        centroids = x[torch.randperm(n, device=x.device, generator=gen)[:nlist]].clone()
        sample = None
        if n > CELLS_SAMPLE * nlist:
            sample = torch.randperm(n, device=x.device, generator=gen)[:CELLS_SAMPLE * nlist]
        xs = x if sample is None else x[sample]
        self._kmeans_init, self._kmeans_sample = centroids.clone(), sample
        for _ in range(iters):
            cell = self._nearest_cell(xs, centroids)
            sums = torch.zeros_like(centroids).index_put_((cell,), xs, accumulate=True)
            count = torch.bincount(cell, minlength=nlist)
            centroids = torch.where(count[:, None] > 0, sums / count.clamp(min=1)[:, None].to(sums.dtype), centroids)
        return centroids

    def _probe(self, q: torch.Tensor):
        """(probes (m, nprobe) int32 unordered, nearest (m) int64) of centred, padded queries."""
        m = q.shape[0]
        probes = torch.empty((m, self.nprobe), dtype=torch.int32, device=q.device)
        nearest = torch.empty(m, dtype=torch.int64, device=q.device)
        vals = torch.empty((min(m, 65536), self.nprobe), dtype=torch.float32, device=q.device)
        rows = max(1, min(65536, (1 << 26) // self.nlist))
        for s in range(0, m, rows):
            d2 = torch.addmm(self._csq[None, :], q[s:s + rows], self._centroids.T, alpha=-2.0)
            nearest[s:s + rows] = d2.argmin(1)
            _lib.check(_lib.load().mgp_topk_rows_f32(_lib.ptr(d2), d2.shape[0], d2.shape[1], d2.stride(0), self.nprobe,
                                                     _lib.ptr(vals), _lib.ptr(probes[s:s + rows]), _lib.stream_ptr()),
                       "mgp_topk_rows_f32")
        return probes, nearest

    def probe(self, queries: torch.Tensor) -> torch.Tensor:
        """(m, nprobe) int64: the cells the search visits for every query row (unordered)."""
        queries = queries[:, None] if queries.ndim == 1 else queries
        q = self._pad_features(queries.to(self.train.dtype) - self._mean)
        return self._probe(q)[0].to(torch.int64)

    def _cells_nns(self, samples, nn_count, exclude=None):
        """Probe selection, the cell scan, the finish kernel; queries with too few candidates go dense.  Returns the
        caller's row numbers."""
        q = self._pad_features(samples)
        m, k, dev = q.shape[0], int(nn_count), q.device
        idx = torch.empty((m, k), dtype=torch.int64, device=dev)
        dist = torch.empty((m, k), dtype=q.dtype, device=dev)
        self.last_short = torch.zeros((m,), dtype=torch.int32, device=dev)
        if m == 0:
            return idx, dist
        if not 1 <= k <= 64:
            raise ValueError(f"nn_method='ivf' serves 1 <= nn_count <= 64 (k <= 64), got k = {k}")
        probes, nearest = self._probe(q)
        # queries in order of their nearest cell: consecutive workgroups meet the same cells in L2
        order = nearest.argsort()
        qs, ps = q[order].contiguous(), probes[order].contiguous()
        ex = None if exclude is None else exclude.to(torch.int64)[order].contiguous()
        best_d = torch.empty((m, k), device=dev, dtype=torch.float32)
        best_i = torch.empty((m, k), device=dev, dtype=torch.int32)
        short = torch.empty((m,), device=dev, dtype=torch.int32)
        _lib.check(_lib.load().mgp_knn_cells_scan(
            _lib.ptr(self.train), self.train_count, self._width, _lib.ptr(self.cell_start), self.nlist, _lib.ptr(qs), m,
            _lib.ptr(ps), self.nprobe, _lib.ptr(ex), k, _lib.ptr(best_d), _lib.ptr(best_i), _lib.ptr(short),
            _lib.stream_ptr()), "mgp_knn_cells_scan")
        best_i.clamp_(min=0)  # (the -1 of a short list: that query is recomputed below, the finish kernel reads rows)
        si = torch.empty((m, k), dtype=torch.int64, device=dev)
        sd = torch.empty((m, k), dtype=q.dtype, device=dev)
        _lib.check(_lib.load().mgp_knn_finish_f32(_lib.ptr(qs), _lib.ptr(self.train), self._width, _lib.ptr(best_i), m, k,
                                                  _lib.ptr(self._perm), _lib.ptr(si), _lib.ptr(sd), _lib.stream_ptr()),
                   "mgp_knn_finish_f32")
        redo = short.nonzero().reshape(-1)
        if redo.numel():  # exactly, over the whole table (as the exact scan treats its overflow flags)
            ri, rd = self._dense_nns(qs[redo], k, None if ex is None else ex[redo])
            si[redo], sd[redo] = self._perm[ri], rd
        idx[order], dist[order], self.last_short[order] = si, sd, short
        return idx, dist

    # ---- the grid walk (nn_method="exact", algorithm="grid") ---------------------------------------------------------

    @staticmethod
    def _check_grid(train, nn_count, edges, cell_rows):
        """The grid scan's contract (include/muygpys_hip.h: mgp_knn_grid_scan) as ValueErrors that name the limit; no
        other algorithm steps in.  Looks at shapes, dtypes and the caller's edges only: any device."""
        table = train[:, None] if train.ndim == 1 else train
        n, d = table.shape
        k = int(nn_count)
        if table.dtype != torch.float32:
            raise ValueError(f"algorithm='grid' serves float32 tables only (fp32 only), got {table.dtype}")
        if not 1 <= d <= GRID_MAX_D:
            raise ValueError(f"algorithm='grid' serves 1 to {GRID_MAX_D} features (1 <= d <= {GRID_MAX_D}), got d = {d}")
        if not 1 <= k <= 64:
            raise ValueError(f"algorithm='grid' serves 1 <= nn_count <= 64 (k <= 64), got k = {k}")
        if not 1 <= n < 2**31:
            raise ValueError(f"algorithm='grid' serves 1 <= n < 2^31 table rows, got n = {n}")
        if not float(cell_rows) > 0:
            raise ValueError(f"algorithm='grid' takes cell_rows > 0 (mean rows per cell), got {cell_rows}")
        if isinstance(edges, str):
            if edges not in ("uniform", "quantile"):
                raise ValueError(f"algorithm='grid' takes edges='uniform', 'quantile' or a list of d edge tensors, got {edges!r}")
            return
        if len(edges) != d:
            raise ValueError(f"algorithm='grid' takes one edge tensor per feature, got {len(edges)} for d = {d}")
        cells = 1
        for a, e in enumerate(edges):
            e = torch.as_tensor(e).reshape(-1)
            if e.numel() and not (bool(torch.isfinite(e).all()) and bool((e[1:] >= e[:-1]).all())):
                raise ValueError(f"algorithm='grid' takes finite, sorted (non-decreasing) edges; axis {a}'s are not")
            cells *= e.numel() + 1
        if cells > GRID_MAX_CELLS:
            raise ValueError(f"algorithm='grid' serves at most 2^24 cells, got {cells}")

    def _init_grid(self, train, nn_count, edges, cell_rows, chunk):
        table = train[:, None] if train.ndim == 1 else train
        n, d = table.shape
        k = int(nn_count)
        self.train_count, self.feature_count = n, d
        self.nn_count, self.nn_method, self.algorithm, self.chunk = k, "exact", "grid", int(chunk)
        self.use_scan, self.scan_kind, self.last_overflow, self.last_route = False, None, None, None
        self.last_shells = None  # per query: the radius, in cells, of the last shell its walk took (device int32)
        self.last_short = None   # per query: 1 where fewer than k rows had a distance that is a number (a NaN query)
        self.cell_rows = float(cell_rows)
        self._width = 4
        self._mean = table.double().mean(0).to(table.dtype)
        x = self._pad_features(table - self._mean)
        if isinstance(edges, str):
            lo, hi = x[:, :d].min(0).values.double(), x[:, :d].max(0).values.double()
            dims = grid_dims(n, (hi - lo).cpu().tolist(), self.cell_rows)
            per_axis = []
            for a in range(d):
                inner = torch.arange(1, dims[a], device=x.device)
                if edges == "uniform":  # the bounding box in equal parts (fp64, then rounded once: non-decreasing)
                    e = (lo[a] + inner.double() * ((hi[a] - lo[a]) / dims[a])).to(x.dtype)
                else:                   # per-axis quantiles: equal counts along each axis
                    e = x[:, a].sort().values[(inner * n) // dims[a]]
                per_axis.append(e.contiguous())
        else:
            # the caller's edges, shifted like the table (monotone: a row below an edge stays at or below it)
            per_axis = [(torch.as_tensor(e, device=x.device).reshape(-1).to(x.dtype) - self._mean[a]).contiguous()
                        for a, e in enumerate(edges)]
            dims = tuple(int(e.numel()) + 1 for e in per_axis) + (1,) * (3 - d)
        self.grid_shape = dims
        self._edges = per_axis + [None] * (3 - d)
        self._edges_flat = torch.cat(per_axis).contiguous()
        cells = grid_linear(grid_cells(x, self._edges), dims)
        self._perm, self._inv, self.cell_start = cell_layout(cells, dims[0] * dims[1] * dims[2])
        self.train = x[self._perm].contiguous()

    def _grid_scan(self, q, qcell, k, self_pos=None):
        """mgp_knn_grid_scan on centred, padded queries and their per-axis cells (m, 3) int32, in the order given:
        (best_d, best_i (stored positions, unordered), shells)."""
        m, dev = q.shape[0], q.device
        best_d = torch.empty((m, k), device=dev, dtype=torch.float32)
        best_i = torch.empty((m, k), device=dev, dtype=torch.int32)
        shells = torch.empty((m,), device=dev, dtype=torch.int32)
        g0, g1, g2 = self.grid_shape
        _lib.check(_lib.load().mgp_knn_grid_scan(
            _lib.ptr(self.train), self.train_count, _lib.ptr(self.cell_start), g0, g1, g2, _lib.ptr(self._edges_flat),
            _lib.ptr(q), m, _lib.ptr(qcell), _lib.ptr(self_pos), k, _lib.ptr(best_d), _lib.ptr(best_i), _lib.ptr(shells),
            _lib.stream_ptr()), "mgp_knn_grid_scan")
        return best_d, best_i, shells

    def _grid_nns(self, samples, nn_count, exclude=None):
        """The queries' cells, the walk in order of linear cell id (consecutive workgroups meet the same cells in L2), the
        finish kernel.  Returns the caller's row numbers."""
        q = self._pad_features(samples)
        m, k, dev = q.shape[0], int(nn_count), q.device
        idx = torch.empty((m, k), dtype=torch.int64, device=dev)
        dist = torch.empty((m, k), dtype=q.dtype, device=dev)
        if not 1 <= k <= 64:
            raise ValueError(f"algorithm='grid' serves 1 <= nn_count <= 64 (k <= 64), got k = {k}")
        have = self.train_count - (0 if exclude is None else 1)
        if k > have:
            raise ValueError(f"algorithm='grid': nn_count = {k} neighbours of a table that can give {have} "
                             f"(n = {self.train_count}{', the query row excluded' if exclude is not None else ''})")
        # (a refused search leaves the record of the last served one as it is)
        self.last_shells = torch.zeros((m,), dtype=torch.int32, device=dev)
        self.last_short = torch.zeros((m,), dtype=torch.int32, device=dev)
        if m == 0:
            return idx, dist
        qcell = grid_cells(q, self._edges)
        order = grid_linear(qcell, self.grid_shape).argsort()
        qs, cs = q[order].contiguous(), qcell[order].contiguous()
        ex = None if exclude is None else exclude.to(torch.int64)[order].contiguous()
        _, best_i, shells = self._grid_scan(qs, cs, k, ex)
        # -1: fewer than k rows at a distance that is a number (a NaN feature in the query, or in the table's mean).
        # The finish kernel reads rows, so such an entry becomes stored row 0 -- and the query is flagged in last_short
        short = (best_i < 0).any(1).to(torch.int32)
        best_i.clamp_(min=0)
        si = torch.empty((m, k), dtype=torch.int64, device=dev)
        sd = torch.empty((m, k), dtype=q.dtype, device=dev)
        _lib.check(_lib.load().mgp_knn_finish_f32(_lib.ptr(qs), _lib.ptr(self.train), self._width, _lib.ptr(best_i), m, k,
                                                  _lib.ptr(self._perm), _lib.ptr(si), _lib.ptr(sd), _lib.stream_ptr()),
                   "mgp_knn_finish_f32")
        idx[order], dist[order], self.last_shells[order], self.last_short[order] = si, sd, shells, short
        return idx, dist
