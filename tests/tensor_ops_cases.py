"""Case tables, launch-route restatement, references and error bounds for the per-function tensor kernels of
csrc/mgp_tensor_ops.hip (numpy only: importable without a GPU).  tests/test_tensor_ops_cases_cpu.py checks the tables
and the references here; tests/test_gpu_tensor_ops_edges.py runs every case through the C ABI.

Routes.  `route(entry, itemsize, d, k, aligned)` restates the launchers (line numbers of csrc/mgp_tensor_ops.hip):

    crosswise_diffs   :541-556   vec  iff d % E == 0 and fq, fn, out 16-byte aligned, E = 16 / itemsize; else scalar
    pairwise_diffs    :557-571   vec  iff d % E == 0 and f, out 16-byte aligned; else scalar
    pairwise_dists    :581-620   k <= 64 and d <= 64: wave_np{32,64}_s{1..4}_{vec,scalar}: NP = 32 iff k <= 32,
                                 s = ceil(d / 16) blocks of 16 features (DG = s * 16 / E groups of 16 bytes),
                                 vec iff d % E == 0 and f 16-byte aligned;
                                 else tile iff k * (d | 1) * itemsize <= 40960; else thread
    table_pack        :744-762   vec  iff d % E == 0, stride % 16 == 0 and feat, out 16-byte aligned; else scalar
    crosswise_dists, reduce_diffs (:572-580, :621-627)  rows8: 8 lanes per output row, no variants
    kernel_apply, perturb (:628-642)                     elementwise
    loss_sums, column_sums (:643-679)                    reduce

Grid caps.  `grid_cap` is the number of work items one pass of the grid covers (a work item is what one thread, one
8-lane group, one wave task or one workgroup takes per pass); a case with more items than that makes the kernel
stride.  grid_1d (:15-19) caps at kAssumedCus * 32 = 8192 blocks of 256 threads; the reductions at kReduceBlocks = 1024
blocks (:649-650, :665-667); the LDS kernels at capacity_grid of csrc/mgp_launch.h:36-48.

References are evaluated from the inputs as rounded to the dtype under test, in fp64 for fp32 and in np.longdouble
(eps <= 2^-63, asserted) for fp64.  With u = 2^-24 (fp32) or 2^-53 (fp64) the bounds are

    diffs, perturb, table_pack   exact: the same-dtype numpy result bit for bit
    F2 distances     |got - ref| <= (d + 3) u ref: the rounded difference counts twice in its square, one rounding
                     for the square, d - 1 for the additions; any summation order and FMA contraction stays inside
    l2               (d / 2 + 2.5) u ref: the correctly rounded square root halves the relative error and rounds once
    reduce_diffs with a length scale   d + 5 and d / 2 + 3.5 (the quotient's rounding counts twice in the square)
    kernel functions |got - ref| <= (8 + 3 t) u ref while exp(-t) is a normal number, t the exponential's argument:
                     t carries up to three roundings, which the exponential multiplies by t; 8 covers the device
                     exp (1 ulp = 2 u) and the polynomial's roundings.  Beyond: 0 <= got <= the value at the range's
                     end, finite.  The scale enters the reference as the kernel receives it: rounded to the dtype.
    reductions       |got_i - ref_i| <= (m + 8) 2^-53 sum_t mag_i(t), m the additions on the longest path:
                     ceil(n / (256 g)) per thread + 6 (wave) + 4 (workgroup) + ceil(g / 256) + 8 (second stage, g
                     partials); without scratch the g partials meet in one chain of atomics: + g instead of the last
                     two.  8 roundings for one term.  mag_i(t) is |term| where the term is a product or quotient of
                     its inputs (sums 0, 4, column sums).  Where the reference's own formula subtracts or adds rounded
                     intermediates the roundings are relative to those operands, not to the result, so mag takes
                     the operands: hd^2 (sqrt(1 + x^2) + 1) for the pseudo-Huber term hd^2 (sqrt(1 + x^2) - 1);
                     r^2 / sv + |log sv| for the lool term; both for looph; and + 1 for a log(s v) with a scale
                     given, whose rounded product s v moves the logarithm by up to u absolutely (with scale NULL the
                     product is exact).  ref is math.fsum over the wide terms, each split into two doubles.
                     (Measured on an MI355X with sum |term| in place of the operands' magnitudes: error / bound up
                     to 1.89 for the pseudo-Huber sum and 2.83 for looph at small residuals, 0.35 and below for the
                     others -- the cancellation is the formula's, which the kernel restates in fp64 as numpy does;
                     `loss_sums_result_relative_bound` keeps that figure in the test's output.)
"""

import math
import types
import zlib

import numpy as np

ENTRIES = ("crosswise_diffs", "pairwise_diffs", "crosswise_dists", "reduce_diffs", "pairwise_dists", "kernel_apply",
           "perturb", "loss_sums", "column_sums", "table_pack")
DTYPES = ("f32", "f64")
ITEMSIZE = {"f32": 4, "f64": 8}
NP_DTYPE = {"f32": np.float32, "f64": np.float64}
UNIT = {"f32": 2.0 ** -24, "f64": 2.0 ** -53}
METRICS = ("l2", "F2")
KERNELS = ("rbf", "matern05", "matern15", "matern25", "maternInf")  # ids 0 .. 4 of the header, in order
HUBER_DELTA, LOOPH_DELTA = 1.5, 3.0
GUARD = 64  # sentinel elements on either side of every output

ASSUMED_CUS = 256           # mgp_launch.h:24
BLOCK = 256                 # kBlock, mgp_tensor_ops.hip:13
ELEMENTWISE_CAP = ASSUMED_CUS * 32 * BLOCK     # 2 097 152 threads (grid_1d)
ROWS8_CAP = ELEMENTWISE_CAP // 8               # 262 144 rows, 8 lanes each
REDUCE_BLOCKS = 1024        # kReduceBlocks, :426
SCRATCH_DOUBLES = REDUCE_BLOCKS * 6            # mgp_reduce_scratch_doubles, :717
CU_LDS, LDS_GRANULE = 160 * 1024, 1280         # mgp_launch.h:19-21
TILE_LDS_LIMIT = 40 * 1024                     # :613


def wide(dtype):
    """The reference's arithmetic type: at least 10 bits wider than the dtype under test."""
    if dtype == "f32":
        return np.float64
    assert np.finfo(np.longdouble).eps <= 2.0 ** -63, "np.longdouble is not an extended type on this machine"
    return np.longdouble


def vec_elems(itemsize):
    return 16 // itemsize


# ---- launch rules -------------------------------------------------------------------------------------------------------

def route(entry, itemsize, d, k, aligned, stride=None):
    """The kernel form a call takes.  `aligned`: every pointer the launcher looks at is 16-byte aligned.  `stride`:
    table_pack's row stride in bytes."""
    E = vec_elems(itemsize)
    if entry in ("crosswise_diffs", "pairwise_diffs"):
        return "vec" if d % E == 0 and aligned else "scalar"
    if entry == "table_pack":
        return "vec" if d % E == 0 and stride % 16 == 0 and aligned else "scalar"
    if entry == "pairwise_dists":
        if k <= 64 and d <= 64:
            form = "vec" if d % E == 0 and aligned else "scalar"
            return f"wave_np{32 if k <= 32 else 64}_s{-(-d // 16)}_{form}"
        return "tile" if k * (d | 1) * itemsize <= TILE_LDS_LIMIT else "thread"
    if entry in ("crosswise_dists", "reduce_diffs"):
        return "rows8"
    if entry in ("kernel_apply", "perturb"):
        return "elementwise"
    if entry in ("loss_sums", "column_sums"):
        return "reduce"
    raise KeyError(entry)


def all_routes(entry, itemsize):
    """Every string `route` can return for an entry."""
    if entry in ("crosswise_diffs", "pairwise_diffs", "table_pack"):
        return {"vec", "scalar"}
    if entry == "pairwise_dists":
        return {f"wave_np{np_}_s{s}_{f}" for np_ in (32, 64) for s in (1, 2, 3, 4) for f in ("vec", "scalar")} | {"tile", "thread"}
    return {route(entry, itemsize, 1, 1, True)}


def capacity_grid(lds, max_per_cu):
    per_cu = CU_LDS // (-(-lds // LDS_GRANULE) * LDS_GRANULE)
    return ASSUMED_CUS * max(1, min(max_per_cu, per_cu))


def wave_lds(itemsize, d):
    E = vec_elems(itemsize)
    dg = -(-d // 16) * (16 // E)
    return 64 * (dg * E + E) * itemsize


def reduce_blocks(n, R=None, scratch=False):
    """Workgroups of loss_sums (R None) / column_sums; 0: the call is refused."""
    g = min(max(-(-n // BLOCK), 1), REDUCE_BLOCKS)
    if R is not None and scratch and g * R > SCRATCH_DOUBLES:
        g = SCRATCH_DOUBLES // R
    return g


def grid_cap(entry, itemsize=4, d=1, k=1, R=1, scratch=False, aligned=True, stride=None):
    """Work items one pass of the grid covers."""
    if entry in ("crosswise_diffs", "pairwise_diffs", "kernel_apply", "perturb", "table_pack"):
        return ELEMENTWISE_CAP
    if entry in ("crosswise_dists", "reduce_diffs"):
        return ROWS8_CAP
    if entry == "loss_sums":
        return REDUCE_BLOCKS * BLOCK
    if entry == "column_sums":
        return (SCRATCH_DOUBLES // R if scratch and REDUCE_BLOCKS * R > SCRATCH_DOUBLES else REDUCE_BLOCKS) * BLOCK
    if entry == "pairwise_dists":
        r = route(entry, itemsize, d, k, aligned)
        if r.startswith("wave"):
            return capacity_grid(wave_lds(itemsize, d), 16)
        if r == "tile":
            return capacity_grid(k * (d | 1) * itemsize, 32)
        return ELEMENTWISE_CAP
    raise KeyError(entry)


def packed_row_bytes(d, R, itemsize):
    """mgp_packed_row_bytes (csrc/mgp_capi.hip:501-507)."""
    return (d * itemsize + max(16, R * itemsize) + 63) // 64 * 64


# ---- cases ---------------------------------------------------------------------------------------------------------------

def make_case(entry, dtype, **kw):
    kw.setdefault("mis", ())
    c = types.SimpleNamespace(entry=entry, dtype=dtype, **kw)
    parts = [entry, dtype]
    for key, v in kw.items():
        if key == "mis":
            if v:
                parts.append("mis_" + "+".join(v))
        elif isinstance(v, bool):
            parts.append(key if v else "no_" + key)
        else:
            parts.append(f"{key}{v}")
    c.id = "-".join(parts)
    return c


def case_route(c):
    it = ITEMSIZE[c.dtype]
    return route(c.entry, it, getattr(c, "d", 1), getattr(c, "k", 1), not c.mis, getattr(c, "stride", None))


def work_items(c):
    """Work items of a case, in the unit of `case_cap`."""
    E = vec_elems(ITEMSIZE[c.dtype])
    r = case_route(c)
    if c.entry == "crosswise_diffs":
        return c.b * c.k * (c.d // E if r == "vec" else c.d)
    if c.entry == "pairwise_diffs":
        return c.b * c.k * c.k * (c.d // E if r == "vec" else c.d)
    if c.entry == "crosswise_dists":
        return c.b * c.k
    if c.entry in ("reduce_diffs", "kernel_apply", "loss_sums", "column_sums"):
        return c.n
    if c.entry == "perturb":
        return c.b * c.k * c.k
    if c.entry == "table_pack":
        return c.n * (c.stride // 16 if r == "vec" else c.stride // ITEMSIZE[c.dtype])
    if c.entry == "pairwise_dists":
        if r.startswith("wave"):
            nh = 2 if c.k <= 32 else 1
            return -(-c.b // nh)
        return c.b if r == "tile" else c.b * c.k * c.k
    raise KeyError(c.entry)


def case_cap(c):
    return grid_cap(c.entry, ITEMSIZE[c.dtype], getattr(c, "d", 1), getattr(c, "k", 1), getattr(c, "R", 1),
                    getattr(c, "scratch", False), not c.mis, getattr(c, "stride", None))


def _diffs_cases():
    out = []
    for dt in DTYPES:
        E = vec_elems(ITEMSIZE[dt])
        for entry, names in (("crosswise_diffs", ("fq", "fn", "out")), ("pairwise_diffs", ("f", "out"))):
            for i, d in enumerate((1, 2, 3, 4, 5, 8)):
                for j, (b, k) in enumerate(((1, 1), (3, 5), (2, 33))):
                    kw = dict(d=d, b=b, k=k)
                    if entry == "crosswise_diffs":
                        kw["bidx"] = (i + j) % 2 == 0
                    out.append(make_case(entry, dt, **kw))
            # every named pointer off by one element, alone, at a d the vector form would take
            for d in (E, 2 * E):
                for name in names:
                    kw = dict(d=d, b=3, k=5, mis=(name,))
                    if entry == "crosswise_diffs":
                        kw["bidx"] = d == E
                    out.append(make_case(entry, dt, **kw))
        # at the grid cap and past it, both forms (d = E: vec, d = 1 / 3: scalar)
        out += [make_case("crosswise_diffs", dt, d=E, b=ELEMENTWISE_CAP // 2, k=2, bidx=True),
                make_case("crosswise_diffs", dt, d=E, b=ELEMENTWISE_CAP // 2 + 2, k=2, bidx=True),
                make_case("crosswise_diffs", dt, d=1, b=ELEMENTWISE_CAP // 2, k=2, bidx=False),
                make_case("crosswise_diffs", dt, d=3, b=233024, k=3, bidx=True),
                make_case("pairwise_diffs", dt, d=E, b=ELEMENTWISE_CAP // 4, k=2),
                make_case("pairwise_diffs", dt, d=E, b=ELEMENTWISE_CAP // 4 + 1, k=2),
                make_case("pairwise_diffs", dt, d=1, b=ELEMENTWISE_CAP // 4, k=2),
                make_case("pairwise_diffs", dt, d=3, b=77673, k=3)]
    return out


def _rows8_cases():
    out = []
    for dt in DTYPES:
        for d in (1, 7, 8, 9, 16, 17, 65):
            for metric in METRICS:
                for b, k in ((1, 1), (7, 1), (1, 31), (3, 11)):
                    out.append(make_case("crosswise_dists", dt, d=d, b=b, k=k, metric=metric, bidx=(d + b) % 2 == 0))
                for n in (1, 7, 31, 33):
                    for ls in (False, True):
                        out.append(make_case("reduce_diffs", dt, d=d, n=n, metric=metric, ls=ls))
        for d, metric in ((8, "l2"), (9, "F2")):
            out += [make_case("crosswise_dists", dt, d=d, b=ROWS8_CAP // 4, k=4, metric=metric, bidx=True),
                    make_case("crosswise_dists", dt, d=d, b=52429, k=5, metric=metric, bidx=True),
                    make_case("reduce_diffs", dt, d=d, n=ROWS8_CAP, metric=metric, ls=d == 8),
                    make_case("reduce_diffs", dt, d=d, n=ROWS8_CAP + 1, metric=metric, ls=d == 9)]
    return out


PD_K = (1, 2, 31, 32, 33, 63, 64)
PD_D = (1, 3, 4, 15, 16, 17, 32, 33, 48, 49, 63, 64)


def _pairwise_dists_cases():
    out = []
    for dt in DTYPES:
        it = ITEMSIZE[dt]
        E = vec_elems(it)
        n = 0
        # every d with both NP; where the vector form exists, also with f off by one element (the scalar gather)
        for d in PD_D:
            for ks in ((1, 2, 31, 32), (33, 63, 64)):
                for mis in ((), ("f",)) if d % E == 0 else ((),):
                    out.append(make_case("pairwise_dists", dt, d=d, k=ks[n % len(ks)], b=1 + n % 3, metric=METRICS[n % 2], mis=mis))
                    n += 1
        # every k with b = 1, 2, 3 (b = 3: an odd last task at two neighbourhoods per wave), at 2, 3 and 4 blocks of 16 features
        for k in PD_K:
            for b in (1, 2, 3):
                out.append(make_case("pairwise_dists", dt, d=(32, 48, 64)[b - 1], k=k, b=b, metric=METRICS[(k + b) % 2]))
        # the wave kernels at and past their capacity grid
        cap = grid_cap("pairwise_dists", it, d=4, k=3)
        out += [make_case("pairwise_dists", dt, d=4, k=3, b=2 * cap, metric="l2"),
                make_case("pairwise_dists", dt, d=4, k=3, b=2 * cap + 1, metric="F2"),
                make_case("pairwise_dists", dt, d=3, k=33, b=grid_cap("pairwise_dists", it, d=3, k=33) + 1, metric="l2")]
        # tile: both sides of k <= 64 and d <= 64, the largest k at d = 65 inside 40 KiB, an even d (d | 1 != d)
        kmax = TILE_LDS_LIMIT // (65 * it)
        for k, d, b in ((65, 1, 2), (65, 64, 3), (1, 65, 2), (64, 65, 1), (kmax, 65, 2), (70, 66, 2)):
            out.append(make_case("pairwise_dists", dt, d=d, k=k, b=b, metric=METRICS[(k + d) % 2]))
        cap = grid_cap("pairwise_dists", it, d=65, k=2)
        out += [make_case("pairwise_dists", dt, d=65, k=2, b=cap, metric="F2"),
                make_case("pairwise_dists", dt, d=65, k=2, b=cap + 1, metric="l2")]
        # thread: one k above the tile's limit; at and past grid_1d's cap
        out += [make_case("pairwise_dists", dt, d=65, k=kmax + 1, b=2, metric="l2"),
                make_case("pairwise_dists", dt, d=65, k=kmax + 1, b=2, metric="F2"),
                make_case("pairwise_dists", dt, d={4: 10, 8: 6}[it], k=1024, b=2, metric="F2"),
                make_case("pairwise_dists", dt, d={4: 10, 8: 6}[it], k=1024, b=3, metric="l2")]
    return out


def _kernel_apply_cases():
    out = []
    for dt in DTYPES:
        for kernel in KERNELS:
            for scale in (1.0, 0.37):
                out += [make_case("kernel_apply", dt, kernel=kernel, scale=scale, n=1),
                        make_case("kernel_apply", dt, kernel=kernel, scale=scale, n=257)]
        out += [make_case("kernel_apply", dt, kernel="matern25", scale=0.37, n=ELEMENTWISE_CAP),
                make_case("kernel_apply", dt, kernel="matern25", scale=0.37, n=ELEMENTWISE_CAP + 1),
                make_case("kernel_apply", dt, kernel="rbf", scale=1.0, n=ELEMENTWISE_CAP + 1)]
    return out


def _perturb_cases():
    out = []
    for dt in DTYPES:
        for mode in ("scalar", "batch"):
            for k in (1, 2, 64, 65):
                for b in (1, 3):
                    out.append(make_case("perturb", dt, mode=mode, k=k, b=b))
        out += [make_case("perturb", dt, mode="scalar", k=256, b=32), make_case("perturb", dt, mode="batch", k=256, b=33),
                make_case("perturb", dt, mode="scalar", k=256, b=33)]
    return out


def _loss_sums_cases():
    out = []
    for dt in DTYPES:
        for i, n in enumerate((1, 63, 64, 255, 256, 257, 262144, 262145)):
            for j, (var, scale) in enumerate(((False, False), (True, False), (True, True))):
                for scratch in (True, False):
                    if n >= 262144 and (i + j) % 2 and not scratch:
                        continue
                    out.append(make_case("loss_sums", dt, n=n, var=var, scale=scale, scratch=scratch))
        out += [make_case("loss_sums", dt, n=257, var=True, scale=True, scratch=True, equal=True),
                make_case("loss_sums", dt, n=257, var=True, scale=False, scratch=False, equal=True),
                make_case("loss_sums", dt, n=1000, var=True, scale=True, scratch=True, spread=True),
                make_case("loss_sums", dt, n=1000, var=True, scale=False, scratch=False, spread=True)]
    return out


def _column_sums_cases():
    out = []
    for dt in DTYPES:
        for R in (1, 2, 6, 7, 16):
            for n in (1, 255, 257, 300001):
                for scratch in (True, False):
                    out.append(make_case("column_sums", dt, R=R, n=n, scratch=scratch))
            # exactly one pass of the grid this R gets
            out.append(make_case("column_sums", dt, R=R, n=grid_cap("column_sums", R=R, scratch=True), scratch=True))
    return out


def _table_pack_cases():
    out = []
    for dt in DTYPES:
        it = ITEMSIZE[dt]
        E = vec_elems(it)
        m = 0
        for d in (E, 2 * E, E + 1, 1):
            for R in (0, 1, E - 1, E, E + 1):
                strides = ((d + R) * it, packed_row_bytes(d, R, it), -(-(d + R) * it // 16) * 16 + 32)
                for stride in strides:
                    out.append(make_case("table_pack", dt, d=d, R=R, stride=stride, n=(1, 3)[m % 2]))
                    m += 1
        for d in (E, 2 * E):
            for name in ("feat", "out"):
                out.append(make_case("table_pack", dt, d=d, R=1, stride=packed_row_bytes(d, 1, it), n=3, mis=(name,)))
        out += [make_case("table_pack", dt, d=E, R=1, stride=64, n=ELEMENTWISE_CAP // 4),
                make_case("table_pack", dt, d=E, R=1, stride=64, n=ELEMENTWISE_CAP // 4 + 1),
                make_case("table_pack", dt, d=1, R=1, stride=2 * it, n=ELEMENTWISE_CAP // 2),
                make_case("table_pack", dt, d=1, R=1, stride=2 * it, n=ELEMENTWISE_CAP // 2 + 1)]
    return out


def _unique(cases):
    seen, out = set(), []
    for c in cases:
        if c.id not in seen:
            seen.add(c.id)
            out.append(c)
    return out


CASES = _unique(_diffs_cases() + _rows8_cases() + _pairwise_dists_cases() + _kernel_apply_cases() + _perturb_cases()
                + _loss_sums_cases() + _column_sums_cases() + _table_pack_cases())


def cases_of(entry):
    return [c for c in CASES if c.entry == entry]


def alloc_bytes(c):
    """Device bytes a case allocates: inputs, indices, the output with its sentinels, scratch."""
    it = ITEMSIZE[c.dtype]
    e = c.entry
    if e == "crosswise_diffs":
        return it * (2 * TABLE_ROWS * c.d + (0 if c.bidx else c.b * c.d) + c.b * c.k * c.d + 2 * GUARD + 3) + 8 * c.b * (c.k + 1)
    if e == "pairwise_diffs":
        return it * (TABLE_ROWS * c.d + c.b * c.k * c.k * c.d + 2 * GUARD + 2) + 8 * c.b * c.k
    if e == "crosswise_dists":
        return it * (2 * TABLE_ROWS * c.d + (0 if c.bidx else c.b * c.d) + c.b * c.k + 2 * GUARD) + 8 * c.b * (c.k + 1)
    if e == "reduce_diffs":
        return it * (c.n * c.d + c.d + c.n + 2 * GUARD)
    if e == "pairwise_dists":
        return it * (TABLE_ROWS * c.d + 1 + c.b * c.k * c.k + 2 * GUARD) + 8 * c.b * c.k
    if e == "kernel_apply":
        return it * (2 * c.n + 2 * GUARD)
    if e == "perturb":
        return it * (2 * c.b * c.k * c.k + c.b * c.k + 2 * GUARD)
    if e == "loss_sums":
        return it * 3 * c.n + 8 * (1 + 6 + 2 * GUARD + SCRATCH_DOUBLES)
    if e == "column_sums":
        return it * c.n * c.R + 8 * (c.R + 2 * GUARD + SCRATCH_DOUBLES)
    if e == "table_pack":
        return it * (c.n * (c.d + c.R) + 2 * GUARD + 2) + c.n * c.stride
    raise KeyError(e)


# ---- inputs --------------------------------------------------------------------------------------------------------------

TABLE_ROWS = 41  # rows of a feature table (indices cover 0 and TABLE_ROWS - 1, with repeats)


def _rng(c):
    return np.random.default_rng(zlib.crc32(c.id.encode()))


def _indices(rng, shape, n):
    idx = rng.integers(0, n, size=shape, dtype=np.int64)
    flat = idx.reshape(-1)
    flat[0] = 0
    flat[-1] = n - 1
    if flat.size >= 4:
        flat[2] = flat[1]  # a repeated index inside the first neighbourhood
    return idx


def kernel_t_end(dtype):
    """The exponential's argument at which exp(-t) leaves the normal range of the dtype."""
    return -math.log(float(np.finfo(NP_DTYPE[dtype]).tiny))


def _kernel_x_of_t(kernel, t, scale):
    div = {"rbf": 0.5, "matern05": 1.0, "matern15": math.sqrt(3.0), "matern25": math.sqrt(5.0)}
    if kernel == "maternInf":
        return np.sqrt(2.0 * t) / scale
    return t / (div[kernel] * scale)


def make_inputs(c):
    """The numpy inputs of a case, in the dtype under test (deterministic in the case id)."""
    rng, T, e = _rng(c), NP_DTYPE[c.dtype], c.entry
    s = types.SimpleNamespace()
    normal = lambda *shape: rng.standard_normal(shape).astype(T)
    if e in ("crosswise_diffs", "crosswise_dists"):
        s.fn = normal(TABLE_ROWS, c.d)
        s.nidx = _indices(rng, (c.b, c.k), TABLE_ROWS)
        if c.bidx:
            s.fq, s.bidx = normal(TABLE_ROWS, c.d), _indices(rng, (c.b,), TABLE_ROWS)
        else:
            s.fq, s.bidx = normal(c.b, c.d), None
    elif e in ("pairwise_diffs", "pairwise_dists"):
        s.f = normal(TABLE_ROWS, c.d)
        s.nidx = _indices(rng, (c.b, c.k), TABLE_ROWS)
    elif e == "reduce_diffs":
        s.diffs = normal(c.n, c.d)
        s.ls = (0.5 + 2.0 * rng.random(c.d)).astype(T) if c.ls else None
    elif e == "kernel_apply":
        t_end = kernel_t_end(c.dtype)
        if c.n == 1:
            x = np.array([0.7])
        else:
            beyond = np.array([1.05, 1.5, 10.0]) * t_end
            t = np.concatenate([np.geomspace(1e-8, 0.999 * t_end, c.n - 1 - beyond.size), beyond])
            # 0, a log-spaced grid of the exponential's argument up to the end of the normal range, three beyond it
            x = np.concatenate([[0.0], _kernel_x_of_t(c.kernel, t, float(T(c.scale)))])
        s.x = x.astype(T)
    elif e == "perturb":
        s.Kin = normal(c.b, c.k, c.k)
        s.eps = 0.1 + 1e-3 * float(rng.random())
        s.noise = (1e-3 + rng.random((c.b, c.k))).astype(T) if c.mode == "batch" else None
    elif e == "loss_sums":
        s.target = normal(c.n)
        s.pred = s.target.copy() if getattr(c, "equal", False) else normal(c.n)
        s.var = s.scale = None
        if c.var:
            if getattr(c, "spread", False):
                s.var = (10.0 ** rng.uniform(-30.0, 6.0, c.n)).astype(T)
            else:
                s.var = (0.05 + rng.random(c.n)).astype(T)
        if c.scale:
            s.scale = np.array([1.7 + float(rng.random())])
    elif e == "column_sums":
        s.x = normal(c.n, c.R)
    elif e == "table_pack":
        s.feat = normal(c.n, c.d)
        s.targets = normal(c.n, c.R) if c.R else None
    else:
        raise KeyError(e)
    return s


# ---- references ----------------------------------------------------------------------------------------------------------

def ref_crosswise_diffs(fq, fn, bidx, nidx):
    """_src/gp/tensors/numpy.py:47-58 in the dtype itself: the kernel's result bit for bit."""
    q = fq[bidx] if bidx is not None else fq[: nidx.shape[0]]
    return q[:, None, :] - fn[nidx]


def ref_pairwise_diffs(f, nidx):
    """:61-69."""
    p = f[nidx]
    return p[:, :, None, :] - p[:, None, :, :]


def ref_metric(diffs_wide, metric):
    """:89-94, _F2 / _l2."""
    f2 = np.sum(diffs_wide * diffs_wide, axis=-1)
    return np.sqrt(f2) if metric == "l2" else f2


def dist_bound(ref, d, metric, dtype, with_ls=False):
    u = UNIT[dtype]
    coeff = (d / 2.0 + 2.5 if metric == "l2" else d + 3.0) + ((1.0 if metric == "l2" else 2.0) if with_ls else 0.0)
    return coeff * u * ref


def ref_crosswise_dists(c, s):
    W = wide(c.dtype)
    q = s.fq[s.bidx] if s.bidx is not None else s.fq[: c.b]
    ref = ref_metric(q.astype(W)[:, None, :] - s.fn.astype(W)[s.nidx], c.metric)
    return ref, dist_bound(ref, c.d, c.metric, c.dtype)


def ref_pairwise_dists(c, s):
    """(b, k, k) in the wide type, in blocks of at most 4 M differences (the large-b and large-k cases)."""
    W = wide(c.dtype)
    f = s.f.astype(W)
    ref = np.empty((c.b, c.k, c.k), dtype=W)
    bstep = max(1, (1 << 22) // (c.k * c.k * c.d))
    istep = max(1, min(c.k, (1 << 22) // (c.k * c.d)))
    for lo in range(0, c.b, bstep):
        p = f[s.nidx[lo:lo + bstep]]
        for i in range(0, c.k, istep):
            ref[lo:lo + bstep, i:i + istep] = ref_metric(p[:, i:i + istep, None, :] - p[:, None, :, :], c.metric)
    return ref, dist_bound(ref, c.d, c.metric, c.dtype)


def ref_reduce_diffs(c, s):
    W = wide(c.dtype)
    x = s.diffs.astype(W)
    if s.ls is not None:
        x = x / s.ls.astype(W)  # gp/deformation/anisotropy.py:70
    ref = ref_metric(x, c.metric)
    return ref, dist_bound(ref, c.d, c.metric, c.dtype, with_ls=s.ls is not None)


def kernel_argument(kernel, x):
    """The exponential's argument t of a kernel at its (already scaled) input."""
    W = x.dtype.type
    if kernel == "rbf":
        return x / W(2)
    if kernel == "matern05":
        return x
    if kernel == "matern15":
        return x * np.sqrt(W(3))
    if kernel == "matern25":
        return x * np.sqrt(W(5))
    return x * x / W(2)


def kernel_value(kernel, x):
    """_src/gp/kernels/numpy.py:12-31 in the type of x."""
    W = x.dtype.type
    t = kernel_argument(kernel, x)
    if kernel == "matern15":
        return (W(1) + t) * np.exp(-t)
    if kernel == "matern25":
        return (W(1) + t + t * t / W(3)) * np.exp(-t)
    return np.exp(-t)


def ref_kernel_apply(c, s):
    """(ref, bound, inside): `inside` marks the inputs whose exp(-t) is a normal number of the dtype; for the others
    `bound` is unused and `ref_kernel_end` bounds the result from above."""
    W, T = wide(c.dtype), NP_DTYPE[c.dtype]
    x = s.x.astype(W) * W(T(c.scale))
    t = kernel_argument(c.kernel, x)
    ref = kernel_value(c.kernel, x)
    inside = np.exp(-t) >= W(np.finfo(T).tiny)
    return ref, (8.0 + 3.0 * t) * UNIT[c.dtype] * ref, inside


def ref_kernel_end(c):
    """The kernel's value where exp(-t) = the smallest normal number of the dtype."""
    W = wide(c.dtype)
    t = W(kernel_t_end(c.dtype))
    poly = {"matern15": W(1) + t, "matern25": W(1) + t + t * t / W(3)}.get(c.kernel, W(1))
    return poly * np.exp(-t)


def ref_perturb(c, s):
    """_src/gp/noise/numpy.py:9-14 / :56-67 in the dtype itself; off the diagonal the input's own bits."""
    T = NP_DTYPE[c.dtype]
    out = s.Kin.copy()
    i = np.arange(c.k)
    add = s.noise if c.mode == "batch" else T(s.eps)
    out[:, i, i] = s.Kin[:, i, i] + add
    return out


def _fsum_wide(terms):
    """Exact sum of wide terms: every term split into two doubles, math.fsum over all of them."""
    hi = terms.astype(np.float64)
    lo = (terms - hi.astype(terms.dtype)).astype(np.float64)
    return math.fsum(hi.tolist() + lo.tolist())


def reduce_path_adds(n, g, scratch):
    """Additions on the longest path of the two-stage (scratch) or atomic (no scratch) reduction over g workgroups."""
    per_thread = -(-n // (g * BLOCK))
    return per_thread + 6 + 4 + ((-(-g // BLOCK) + 8) if scratch else g)


def loss_terms(pred, target, var, scale, hd=HUBER_DELTA, ld=LOOPH_DELTA):
    """The six per-element terms of mgp_loss_sums (_src/optimize/loss/numpy.py:22-117; sums 4 and 5 are the scale-free
    pieces r^2 / v and log v) and the magnitudes their roundings are relative to (module docstring), in the type of
    `pred`.  var None: terms 1, 3, 4, 5 are zero."""
    W = pred.dtype.type
    r = pred - target
    r2 = r * r
    zero = np.zeros_like(r2)
    x = r / W(hd)
    root2 = np.sqrt(W(1) + x * x)
    terms = [r2, zero, W(hd) * W(hd) * (root2 - W(1)), zero, zero, zero]
    mags = [r2, zero, W(hd) * W(hd) * (root2 + W(1)), zero, zero, zero]
    if var is not None:
        sv = (W(scale) if scale is not None else W(1)) * var
        logsv = np.log(sv)
        prod = W(1) if scale is not None else W(0)  # the rounded product s v under the logarithm
        root3 = np.sqrt(W(1) + r2 / (W(ld) * W(ld) * sv))
        terms[1], mags[1] = r2 / sv + logsv, r2 / sv + np.abs(logsv) + prod
        terms[3] = W(2) * W(ld) * W(ld) * (root3 - W(1)) + logsv
        mags[3] = W(2) * W(ld) * W(ld) * (root3 + W(1)) + np.abs(logsv) + prod
        terms[4] = mags[4] = r2 / var
        terms[5], mags[5] = np.log(var), np.abs(np.log(var))
    return terms, mags


def ref_loss_sums(c, s):
    """(ref, bound): six doubles each.  The reductions run in fp64 for both dtypes, so the wide type is longdouble."""
    W = wide("f64")
    terms, mags = loss_terms(s.pred.astype(W), s.target.astype(W), None if s.var is None else s.var.astype(W),
                             None if s.scale is None else float(s.scale[0]))
    g = reduce_blocks(c.n)
    m = reduce_path_adds(c.n, g, c.scratch)
    ref = np.array([_fsum_wide(t) for t in terms])
    bound = np.array([(m + 8) * 2.0 ** -53 * _fsum_wide(a) for a in mags])
    return ref, bound


def loss_sums_result_relative_bound(c, s):
    """(m + 8) 2^-53 sum |term| with the terms' own values in place of their operands' magnitudes: reported next to the
    asserted bound, never asserted (for sums 1 to 3 it is no bound of the reference's own formula, module docstring)."""
    W = wide("f64")
    terms, _ = loss_terms(s.pred.astype(W), s.target.astype(W), None if s.var is None else s.var.astype(W),
                          None if s.scale is None else float(s.scale[0]))
    m = reduce_path_adds(c.n, reduce_blocks(c.n), c.scratch)
    return np.array([(m + 8) * 2.0 ** -53 * _fsum_wide(np.abs(t)) for t in terms])


def ref_column_sums(c, s):
    g = reduce_blocks(c.n, c.R, c.scratch)
    m = reduce_path_adds(c.n, g, c.scratch)
    x = s.x.astype(np.float64)  # exact for both dtypes
    ref = np.array([math.fsum(x[:, r].tolist()) for r in range(c.R)])
    bound = np.array([(m + 8) * 2.0 ** -53 * math.fsum(np.abs(x[:, r]).tolist()) for r in range(c.R)])
    return ref, bound


def ref_table_pack(c, s):
    """(n, stride / itemsize) in the dtype: [features | responses | zero pad], byte for byte."""
    T = NP_DTYPE[c.dtype]
    out = np.zeros((c.n, c.stride // ITEMSIZE[c.dtype]), dtype=T)
    out[:, :c.d] = s.feat
    if c.R:
        out[:, c.d:c.d + c.R] = s.targets
    return out
