"""The cases of tests/test_gpu_knn_long.py and what they are checked with: the long-row k-NN scans
(mgp_knn_scan_long, mgp_knn_scan_long_wide: csrc/mgp_knn_long.hip) called directly, against fp64 brute force.

Everything here runs on any device: the inputs are drawn and centred on the CPU (the same bits wherever the test runs),
and the no-overflow precondition of the narrow entry is a property of the inputs alone -- `python -m tests.knn_long_cases`
evaluates it in fp64 for every benign narrow case without a GPU (how the seeds were checked before they were committed).

What a call is made of, the reference and the bound are those of tests/test_gpu_knn_scan_edges.py (f32 entry) and
tests/test_gpu_knn_wide.py: the table centred on its fp64 mean (queries shifted alike), squared norms rounded from fp64
and padded with +inf to a multiple of 64, IN lists = the exact k-best over rows [0, start) from torch (Gram form, fp32),
a zero-filled overflow vector; fp64 distances on the same centred fp32 data, self excluded; per query the sorted fp64
distances of the returned rows within 2 e of the sorted true top-k,
    e = (d + 5) 2^-24 (|q|^2 + max_x |x|^2)    (Gram form: an fmaf chain of d products from -|x|^2/2, fp32-rounded norms)
derived, not measured.

Sizes.  Narrow entry: start = max(64, 32 k) rounded to 64 (k = 1, 30, 64: 64, 960, 2 048 head rows) and 701 rows behind
it (eleven tiles, the last one partial); wide entry: start = k + 1 rounded up to 64 and n = 1 400 + (k = 1024: start).
A tile is 64 rows, a workgroup owns 128 queries (four waves of 32).

No overflow (narrow entry, benign cases): the thresholds only tighten, so what can enter a query's 16-entry queue
between two drains is a subset of the rows of that window closer than the query's k-th best over [0, start): at most
QUEUE_ROOM = 12 in every window of tiles a workgroup drains together (`worst_window`, the kernel's own walk and drain
schedule).  RESEED lists the cases whose first draw broke that (at most 2 of the grid)."""

import types
import zlib

import torch

U = 2.0 ** -24      # unit roundoff of fp32
TN = 64             # rows per tile
QB = 128            # queries per workgroup
QUEUE_ROOM = 12     # of the 16 queue entries
SYMBOL = {"narrow": "mgp_knn_scan_long", "wide": "mgp_knn_scan_long_wide"}

WIDTHS = (68, 72, 124, 128, 132, 192, 196, 252, 256)  # first past 64, a last chunk of 4, chunk multiples, one group past
K_OF = {"narrow": (1, 30, 64), "wide": (65, 130, 1024)}
M_ALL = (1, 127, 129, 300)  # a partial wave, a partial workgroup, several workgroups
PAST = 701                  # rows behind `start`, narrow entry: n is no multiple of 64

# cases whose first draw broke the no-overflow precondition: another seed, the same cap (none so far)
RESEED = {}


def start_of(entry, k):
    return max(64, -(-(32 * k) // 64) * 64) if entry == "narrow" else -(-(k + 1) // 64) * 64


def rows_of(entry, k):
    return start_of(entry, k) + PAST if entry == "narrow" else max(1400, start_of(entry, k) + 312)


def case(entry, d, k, m, table="normal", self_mode=None, name="a"):
    return types.SimpleNamespace(entry=entry, d=d, k=k, m=m, table=table, self_mode=self_mode, name=name,
                                 start=start_of(entry, k), n=rows_of(entry, k))


def case_id(c):
    return "-".join(str(v) for v in (c.name, c.entry, f"d{c.d}", f"k{c.k}", f"m{c.m}", c.table, c.self_mode) if v is not None)


def benign_cases(entry):
    ks = K_OF[entry]
    cases = [case(entry, d, k, 129) for d in WIDTHS for k in ks]                            # widths x list lengths
    cases += [case(entry, d, ks[1], m, name="m") for d in (68, 256) for m in M_ALL if m != 129]  # query counts
    cases += [case(entry, d, ks[1], 129, self_mode="rows", name="self") for d in (68, 132, 256)]
    # a dropped or misaligned chunk returns the wrong rows outright
    cases += [case(entry, d, ks[1], 129, table="last4") for d in (68, 132, 196, 256)]
    cases += [case(entry, 68, ks[1], 129, table="cols60_67")]
    # ... and so does a wave half that reads the other half's columns
    cases += [case(entry, d, ks[1], 129, table="tail") for d in (68, 128, 196, 256)]
    return cases


def build(c):
    """(X, Q, self_idx or None) on the CPU, not centred yet."""
    seed_of = case_id(c)
    g = torch.Generator().manual_seed(zlib.crc32(f"{seed_of}#{RESEED.get(seed_of, 0)}".encode()))
    X, Q = torch.randn(c.n, c.d, generator=g), torch.randn(c.m, c.d, generator=g)
    keep = None
    if c.table == "last4":        # the only non-zero features are the last four columns
        keep = slice(c.d - 4, c.d)
    elif c.table == "cols60_67":  # ... are columns 60 .. 67: both sides of the first chunk's end at d = 68
        keep = slice(60, 68)
    elif c.table == "tail":       # equal in the first 64 columns, differing only in columns 64 .. d - 1
        X[:, :64] = X[0, :64]
        Q[:, :64] = X[0, :64]
    if keep is not None:
        mask = torch.zeros(c.d)
        mask[keep] = 1.0
        X, Q = X * mask, Q * mask
    self_idx = None
    if c.self_mode == "rows":  # queries that are table rows, inside and beyond `start`
        half = c.m // 2
        self_idx = torch.cat([torch.randperm(c.start, generator=g)[:half],
                              c.start + torch.randperm(c.n - c.start, generator=g)[:c.m - half]])
        Q = X[self_idx].clone()
    return X, Q, self_idx


def centre(X, Q):
    mean = X.double().mean(0)
    return (X.double() - mean).float().contiguous(), (Q.double() - mean).float().contiguous()


def true_distances(Xc, Qc, self_idx=None):
    """(m, n) fp64 squared distances, +inf at a query's own row."""
    D = torch.cdist(Qc.double(), Xc.double(), compute_mode="donot_use_mm_for_euclid_dist") ** 2
    if self_idx is not None:
        D[torch.arange(D.shape[0], device=D.device), self_idx.to(D.device)] = float("inf")
    return D


def drain_windows(ntiles, block):
    """The tiles workgroup `block` drains together, in walk order: the narrow kernel's own rules."""
    first = block * 7919 % ntiles
    windows, current, next_drain = [], [], 0
    for tj in range(ntiles):
        current.append((first + tj) % ntiles)
        if tj < next_drain and tj + 1 < ntiles:
            continue
        next_drain = tj + (1 if tj < 64 else 4 if tj < 256 else 8 if tj < 1024 else 16)
        windows.append(current)
        current = []
    return windows


def worst_window(D, k, start):
    """The most rows of one drain window that beat a query's initial k-th best, over all queries."""
    m, n = D.shape
    ntiles = -(-(n - start) // TN)
    tau0 = D[:, :start].topk(k, dim=1, largest=False).values[:, -1]
    beats = (D[:, start:] < tau0[:, None]).to(torch.int32)
    beats = torch.nn.functional.pad(beats, (0, ntiles * TN - beats.shape[1]))
    per_tile = beats.reshape(m, ntiles, TN).sum(-1)
    worst = 0
    for block in range(-(-m // QB)):
        mine = per_tile[block * QB:(block + 1) * QB]
        for window in drain_windows(ntiles, block):
            worst = max(worst, int(mine[:, window].sum(1).max()))
    return worst


def gram_error(Xc, Qc):
    """e of the module docstring, one per query."""
    d = Xc.shape[1]
    return (d + 5) * U * ((Qc.double() ** 2).sum(1) + (Xc.double() ** 2).sum(1).max())


if __name__ == "__main__":
    bad = []
    for c in benign_cases("narrow"):
        X, Q, self_idx = build(c)
        Xc, Qc = centre(X, Q)
        worst = worst_window(true_distances(Xc, Qc, self_idx), c.k, c.start)
        print(f"{case_id(c):48s} worst drain window {worst}")
        if worst > QUEUE_ROOM:
            bad.append(case_id(c))
    print("cases to reseed:", bad)
