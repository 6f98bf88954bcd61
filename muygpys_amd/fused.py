"""Fused hot-path entry points (one HIP launch from features + indices to mean/var).

These wrap ``mgp_posterior_{f32,f64}`` of the C ABI.  They are what the lazy tensor
handles of the ``hip`` backend call when a MuyGPyS-style caller runs
``make_predict_tensors -> kernel -> posterior_mean / posterior_variance`` (reference
call stack: gp/muygps.py:406-475, gp/kernels/matern.py:148-168, gp/muygps.py:164-259),
and what ``bench.py`` times.
"""

from __future__ import annotations

import contextlib
import os
from collections import OrderedDict
from dataclasses import dataclass
from typing import NamedTuple, Optional, Sequence, Union

import torch

from . import _lib

Number = Union[int, float]


@dataclass
class KernelSpec:
    """Hyper-parameters of one local-GP model, in the reference's vocabulary.

    kernel: "rbf" | "matern05" | "matern15" | "matern25" | "maternInf"
        (_src/gp/kernels/numpy.py:12-31; Matern with fixed nu, gp/kernels/matern.py:61-81), or
        "matern_gen" with ``smoothness`` = nu (numpy.py:34-43: any 0 < nu <= 30 on the fused path, fp32 and -- since
        round 4 -- fp64 tables; :class:`FusedUnsupported` otherwise, and the caller materialises)
    metric: "l2" | "F2"  (gp/deformation/metric.py:237-265)
    length_scale: scalar -> Isotropy (isotropy.py:60-89); sequence of d -> Anisotropy
        (anisotropy.py:43-70)
    noise: scalar -> HomoscedasticNoise; 1-D tensor (n_train,) -> heteroscedastic table
        gathered with nn_indices (tensors/numpy.py:11-15); 2-D tensor (b, k) ->
        already gathered HeteroscedasticNoise tensor (noise/numpy.py:56-67)
    length_scale_batch: a length scale per neighbourhood, ``(b,)`` / ``(b, 1)`` (Isotropy) or ``(b, d)`` (Anisotropy):
        the nonstationary model (HierarchicalParameter, gp/hyperparameter/experimental/hierarchical.py; the ``(b,)``
        scale divides Kin and Kcross of batch element i alike, isotropy.py:60-89).  Row i belongs to the neighbourhood at
        position i of the batch.  When set, ``length_scale`` is ignored; :func:`posterior_mean_var` alone serves such a
        spec (closed-form kernels), every other consumer raises ``ValueError``.
    """

    kernel: str = "matern15"
    metric: str = "l2"
    length_scale: Union[Number, Sequence[Number], torch.Tensor] = 1.0
    noise: Union[Number, torch.Tensor] = 0.0
    smoothness: Optional[float] = None
    length_scale_batch: Optional[torch.Tensor] = None

    def kernel_id(self) -> int:
        try:
            return _lib.KERNEL_IDS[self.kernel]
        except KeyError:
            raise ValueError(f"unknown kernel {self.kernel!r}; expected one of {sorted(_lib.KERNEL_IDS)}")

    def metric_id(self) -> int:
        try:
            return _lib.METRIC_IDS[self.metric]
        except KeyError:
            raise ValueError(f"unknown metric {self.metric!r}; expected 'l2' or 'F2'")


class FusedUnsupported(RuntimeError):
    """The fused kernels do not serve this model / shape (general-smoothness Matern beyond nu = 30, with 33 to 64
    slots in a batch too small to compile a kernel for, with more than 1024 rows ...): evaluate through the
    per-function kernels instead."""


# device-resident length scales of host-valued hyper-parameters, keyed by (values, device, dtype): an
# optimiser revisits the same KernelSpec values for mean, variance and scale of one evaluation, and
# a prediction / benchmark loop calls with one spec many times -- no host-to-device copy per call
_LS_CACHE: "OrderedDict[tuple, torch.Tensor]" = OrderedDict()
_LS_CACHE_SIZE = 64


def _length_scale_tensor(ls, d: int, like: torch.Tensor, detach: bool = True) -> torch.Tensor:
    if isinstance(ls, torch.Tensor):
        t = (ls.detach() if detach else ls).to(device=like.device, dtype=like.dtype).reshape(-1).contiguous()
    else:
        vals = (float(ls),) if isinstance(ls, (int, float)) else tuple(float(v) for v in ls)
        key = (vals, like.device, like.dtype)
        t = _LS_CACHE.get(key)
        if t is None:
            t = torch.tensor(vals, device=like.device, dtype=like.dtype)
            _LS_CACHE[key] = t
            if len(_LS_CACHE) > _LS_CACHE_SIZE:
                _LS_CACHE.popitem(last=False)
        else:
            _LS_CACHE.move_to_end(key)
    if t.numel() != 1 and t.numel() != d:
        raise ValueError(
            f"Difference tensor of shape (..., {d}) must have final dimension size of {t.numel()}"
        )
    return t


def refuse_length_scale_batch(spec: "KernelSpec") -> None:
    """What every consumer of a :class:`KernelSpec` but :func:`posterior_mean_var` does with a spec that carries a
    length scale per neighbourhood: ``ValueError`` -- none may silently use ``length_scale`` instead."""
    if getattr(spec, "length_scale_batch", None) is not None:
        raise ValueError("KernelSpec.length_scale_batch (a length scale per neighbourhood) is served by "
                         "fused.posterior_mean_var alone: no LOOCV launch, gradient, fast-prediction, prepared-table "
                         "or general-smoothness path reads it")


# what a non-zero ``info`` of an NS launch is reported as (``_lib.raise_if_not_spd``): a bad pivot or a bad scale
NS_NOT_SPD = ("posterior with a length scale per neighbourhood (the other possible cause: a length scale that is not "
              "positive and finite)")


def _length_scale_batch_tensor(lsb, b: int, d: int, like: torch.Tensor) -> torch.Tensor:
    """``KernelSpec.length_scale_batch`` as the library reads it: ``(b, 1)`` or ``(b, d)``, contiguous, on the tables'
    device and dtype."""
    if not isinstance(lsb, torch.Tensor):
        raise ValueError("length_scale_batch must be a torch.Tensor of shape (b,), (b, 1) or (b, d)")
    _lib.require_cuda(lsb)
    t = lsb.detach().to(device=like.device, dtype=like.dtype)
    t = t[:, None] if t.ndim == 1 else t
    if t.ndim != 2 or t.shape[0] != b or t.shape[1] not in (1, d):
        raise ValueError(f"length_scale_batch must have shape ({b},), ({b}, 1) or ({b}, {d}), got {tuple(lsb.shape)}")
    return t.contiguous()


class PackedTable:
    """A prepared table (``mgp_table_pack_*``): rows ``[features | responses | pad]`` at a 64-byte
    multiple stride, so that the gather of a neighbour row brings its responses along (two cache
    lines per neighbour instead of three at d = 40, fp32).  Built once per (features, targets) pair
    -- the tables do not change across the objective evaluations of a hyper-parameter search.

    Feature rows that are not whole 16-byte groups (d = 1, 2, 3, 5, 6 ... in fp32; odd d in fp64) are padded with
    zero features up to the next group (``d_kernel``): a zero feature adds nothing to any distance, so the kernels run
    on ``d_kernel`` features (Anisotropy: the padded features get length scale 1) and every shape takes the pipelined
    prepared-table kernels -- the reference's univariate tutorial (d = 1) included."""

    def __init__(self, features: torch.Tensor, targets: Optional[torch.Tensor] = None):
        _lib.require_cuda(features, targets)
        f = (features[:, None] if features.ndim == 1 else features).contiguous()
        t = None
        if targets is not None:
            t = (targets[:, None] if targets.ndim == 1 else targets).to(f.dtype).contiguous()
            if t.shape[0] != f.shape[0]:
                raise ValueError("features and targets differ in row count")
        # the source tensors stay referenced for as long as this table lives: the cache below is keyed on
        # their addresses, which must not be handed to another tensor meanwhile
        self._sources = (features, targets)
        self.n, self.d = f.shape
        group = 16 // f.element_size()
        self.d_kernel = (self.d + group - 1) // group * group
        if self.d_kernel != self.d:
            f = torch.nn.functional.pad(f, (0, self.d_kernel - self.d))
        self.R = 0 if t is None else t.shape[1]
        self.dtype = f.dtype
        self.stride = int(_lib.load().mgp_packed_row_bytes(self.d_kernel, self.R, f.element_size()))
        self.data = torch.empty(self.n * self.stride, dtype=torch.uint8, device=f.device)
        _lib.check(
            _lib.fn("table_pack", f.dtype)(
                _lib.ptr(f), _lib.ptr(t), self.n, self.d_kernel, self.R, _lib.ptr(self.data), self.stride, _lib.stream_ptr()
            ),
            "mgp_table_pack",
        )

    @staticmethod
    def supported(d: int, R: int, k: int, dtype) -> bool:
        es = dtype.itemsize
        dk = (d * es + 15) // 16 * 16 // es  # (rows are padded to whole 16-byte groups)
        if dk > 64:
            return False
        if R * es <= 16 and k + 1 + R <= 64:  # the wave kernels: the responses of a row in one 16-byte slot
            return True
        # fp32 predictions with up to sixteen responses and nn_count <= 64 (BASELINE config 5; round 5): the kernel on the
        # matrix cores' layout reads rows [features | 16 responses] at a 256-byte stride (d = 40)
        return es == 4 and 4 < R <= 16 and k <= 64 and dk >= 8 and (dk + 7) // 8 * 8 != 48

    def kernel_length_scale(self, ls: torch.Tensor) -> torch.Tensor:
        """Per-feature length scales padded to ``d_kernel`` entries (ones: the padded features are all zero)."""
        if ls.numel() == 1 or self.d_kernel == self.d:
            return ls
        return torch.cat([ls, torch.ones(self.d_kernel - self.d, device=ls.device, dtype=ls.dtype)])


# Prepared tables are kept per (features, targets) identity: at most _PACK_CACHE_SIZE entries and
# _PACK_CACHE_BYTES bytes of packed copies (an entry also keeps its source tensors alive -- see
# clear_caches()).  A table packed WITHOUT responses (the query side of a prediction on a separate test
# table: every row is read once per neighbourhood, so its pack is pure overhead kept small, not an
# investment) gets a single slot of its own and never evicts a training table.
_PACK_CACHE: "OrderedDict[tuple, PackedTable]" = OrderedDict()
_PACK_CACHE_SIZE = 4
_PACK_CACHE_BYTES = 8 << 30
_QUERY_PACK: "OrderedDict[tuple, PackedTable]" = OrderedDict()


def _tensor_key(t: Optional[torch.Tensor]):
    return None if t is None else (t.data_ptr(), t._version, tuple(t.shape), t.dtype, t.device)


def pack_table(features: torch.Tensor, targets: Optional[torch.Tensor] = None, query: Optional[bool] = None) -> PackedTable:
    """The prepared table of ``(features, targets)``, cached on the tensors' identity and version
    (an in-place edit of either tensor invalidates the entry).  ``query``: the table serves the query
    side only (default: a table without responses does)."""
    key = (_tensor_key(features), _tensor_key(targets))
    cache = _QUERY_PACK if (targets is None if query is None else query) else _PACK_CACHE
    hit = cache.get(key)
    if hit is None:
        hit = PackedTable(features, targets)
        if cache is _QUERY_PACK:
            cache.clear()
        cache[key] = hit
        while len(cache) > 1 and (len(cache) > _PACK_CACHE_SIZE or sum(t.data.numel() for t in cache.values()) > _PACK_CACHE_BYTES):
            cache.popitem(last=False)
    else:
        cache.move_to_end(key)
    return hit


def clear_caches() -> None:
    """Drop the cached prepared tables (and with them the references to their source tensors) and the
    cached device-resident length scales."""
    _PACK_CACHE.clear()
    _QUERY_PACK.clear()
    _LS_CACHE.clear()


def _check_indices(name: str, idx: Optional[torch.Tensor], n: int) -> None:
    """Reference behaviour for an index outside the table: IndexError from the fancy index
    (_src/gp/tensors/numpy.py:47-69).  Costs a device round trip, so only under
    MUYGPYS_HIP_CHECK_INDICES=1 (debugging a neighbour table built on another data set)."""
    if idx is None or idx.numel() == 0:
        return
    lo, hi = int(idx.amin()), int(idx.amax())
    if lo < 0 or hi >= n:
        raise IndexError(f"{name} holds indices in [{lo}, {hi}] but the table has {n} rows")


def _noise_args(noise, b: int, k: int, like: torch.Tensor):
    if isinstance(noise, torch.Tensor) and noise.ndim >= 1:
        _lib.require_cuda(noise)
        nz = noise.to(dtype=like.dtype).contiguous()
        if nz.ndim == 1:
            if nz.shape[0] != like.shape[0]:
                raise ValueError(
                    f"per-training-point noise table holds {nz.shape[0]} entries for {like.shape[0]} training points"
                )
            return _lib.NOISE_TABLE, 0.0, nz
        if nz.shape != (b, k):
            raise ValueError(f"heteroscedastic noise tensor must have shape {(b, k)}, got {tuple(nz.shape)}")
        return _lib.NOISE_BATCH, 0.0, nz
    return _lib.NOISE_SCALAR, float(noise), None


class _Inputs(NamedTuple):
    """The arguments of a fused call as the library takes them (:func:`_normalize`)."""

    fq: torch.Tensor            # (n_q, d) query features, contiguous (`fn` itself when both sides are one tensor)
    fn: torch.Tensor            # (n, d) neighbour features, contiguous
    bi: Optional[torch.Tensor]  # (b,) int64, or None: neighbourhood i belongs to query row i
    ni: torch.Tensor            # (b, k) int64
    tg: Optional[torch.Tensor]  # (n, R) responses, (b, k, R) when gathered, None when the call reads none
    b: int
    k: int
    d: int
    R: int
    squeeze: bool               # the caller's responses had no response axis: results drop theirs
    ls: torch.Tensor            # (1,) or (d,) length scale(s) on the device
    mode: Optional[int]         # the noise triple of _noise_args (None where the call takes no noise)
    eps: Optional[float]
    nz: Optional[torch.Tensor]


def _normalize(spec: KernelSpec, test_features, train_features, batch_indices, nn_indices, targets=None, *,
               gathered: bool = False, responses: str = "any", want_noise: bool = True, detach: bool = True,
               per_neighbourhood: bool = False) -> _Inputs:
    """The one place where the public arguments of a fused function become what the library reads: 2-D contiguous
    tables, int64 indices, the shape and dtype checks, the length scale(s) and the noise triple.  A new model parameter
    is validated and converted here, once.

    ``responses``: "any", "single" (the LOOCV losses) or "labels" (two or more columns: classification).
    ``want_noise=False`` / ``detach=False``: the differentiable path decodes its noise tensor inside the autograd
    function and keeps a length-scale tensor attached to the graph.
    ``per_neighbourhood``: the caller serves ``spec.length_scale_batch`` (``ls`` is then the ``(b, 1)`` / ``(b, d)``
    tensor on the tables' device and dtype); every other caller refuses a spec that carries one."""
    if not per_neighbourhood:
        refuse_length_scale_batch(spec)
    _lib.require_cuda(test_features, train_features, batch_indices, nn_indices, targets)
    dtype = train_features.dtype
    if test_features.dtype != dtype or (targets is not None and targets.dtype != dtype):
        raise TypeError("features and targets must share one float dtype")
    fn = (train_features[:, None] if train_features.ndim == 1 else train_features).contiguous()
    fq = fn if test_features is train_features else (test_features[:, None] if test_features.ndim == 1 else test_features).contiguous()
    d = fn.shape[1]
    if fq.shape[1] != d:
        raise ValueError("test and train features differ in feature count")
    ni = nn_indices.to(torch.int64).contiguous()
    b, k = ni.shape
    bi = None if batch_indices is None else batch_indices.to(torch.int64).contiguous()
    if bi is not None and bi.shape != (b,):
        raise ValueError("batch_indices must have shape (batch_count,)")
    if bi is None and fq.shape[0] < b:
        raise ValueError(f"{b} neighbourhoods but only {fq.shape[0]} query rows (batch_indices is None)")
    tg, R, squeeze = None, 1, False
    if gathered:
        if tuple(targets.shape[:2]) != (b, k):
            raise ValueError(f"gathered responses must have shape ({b}, {k}[, R]), got {tuple(targets.shape)}")
        squeeze = targets.ndim == 2
        tg = targets.reshape(b, k, -1).contiguous()
        R = tg.shape[2]
    elif targets is not None:
        squeeze = targets.ndim == 1
        tg = (targets[:, None] if squeeze else targets).contiguous()
        R = tg.shape[1]
        if responses == "single" and (tg.ndim != 2 or R != 1):
            raise NotImplementedError("the LOOCV losses are defined for a single response (reference: loss/numpy.py:34-61)")
        if responses == "labels" and (tg.ndim != 2 or R < 2):
            raise NotImplementedError("the classification losses are defined for two or more response columns")
        if tg.shape[0] != fn.shape[0]:
            raise ValueError("train_features and train_targets differ in row count")
    if spec.length_scale_batch is not None:
        ls = _length_scale_batch_tensor(spec.length_scale_batch, b, d, fn)
    else:
        ls = _length_scale_tensor(spec.length_scale, d, fn, detach)
    mode, eps, nz = _noise_args(spec.noise, b, k, fn) if want_noise else (None, None, None)
    return _Inputs(fq, fn, bi, ni, tg, b, k, d, R, squeeze, ls, mode, eps, nz)


def _debug_check_indices(inp: _Inputs) -> None:
    if os.environ.get("MUYGPYS_HIP_CHECK_INDICES") == "1":
        _check_indices("nn_indices", inp.ni, inp.fn.shape[0])
        _check_indices("batch_indices", inp.bi, inp.fq.shape[0])


def _use_packed(packed, inp: _Inputs, features, targets, rows: int, gathered: bool = False, threshold: bool = True) -> bool:
    """Whether a call reads its tables through prepared copies (:class:`PackedTable`): never with ``packed=False``,
    an empty batch or a shape the prepared-table kernels do not serve; ``packed="auto"`` additionally asks that the
    pack pays off -- the table is cached already, or the batch gathers at least a quarter of the ``rows`` a pack
    passes over.  ``threshold=False``: a prepared evaluation (:class:`LoocvPlan`) repeats, so "auto" always packs.
    Gathered responses: the FEATURE rows still come from a prepared table (packed without responses)."""
    R, k = (0, inp.k + inp.R) if gathered else (inp.R, inp.k)
    if packed is False or inp.b <= 0 or not PackedTable.supported(inp.d, R, k, inp.fn.dtype):
        return False
    if packed == "auto" and threshold:
        key = (_tensor_key(features), None if gathered else _tensor_key(targets))
        return key in _PACK_CACHE or inp.b * (inp.k + 1) >= rows // 4
    return True


def _model_args(spec: KernelSpec, ls: torch.Tensor) -> tuple:
    """kernel id (the general-smoothness entries: the smoothness instead), metric id, length scale(s) and their count."""
    model = float(spec.smoothness) if spec.kernel == "matern_gen" else spec.kernel_id()
    return (model, spec.metric_id(), _lib.ptr(ls), ls.numel())


def _plain_args(inp: _Inputs, model: tuple, outs: tuple, targets_batch=None) -> tuple:
    """What every posterior entry on the plain tables starts with, in the ABI's order: tables, shape, responses
    (``targets_batch`` behind them where the entry takes it), noise triple, ``model`` (:func:`_model_args`), outputs."""
    P = _lib.ptr
    head = (P(inp.fq), P(inp.fn), inp.d, P(inp.bi), P(inp.ni), inp.b, inp.k, P(inp.tg), inp.R)
    if targets_batch is not None:
        head += (int(targets_batch),)
    return head + (inp.mode, inp.eps, P(inp.nz)) + model + outs[:4]


def _posterior_plain(base: str, inp: _Inputs, model: tuple, outs: tuple, targets_batch=None, slab: bool = False) -> int:
    """One launch of ``mgp_<base>_*`` on the plain tables (``outs`` as for :func:`_posterior_call`); returns the status.
    ``slab``: a ``*_large_*`` entry (csrc/mgp_large.hip), its workspace allocated here; ``ValueError`` beyond 1024 rows."""
    args = _plain_args(inp, model, outs, targets_batch)
    if not slab:
        return _lib.fn(base, inp.fn.dtype)(*args, outs[4])
    ws = _lib.large_workspace(inp.fn.dtype, inp.k, inp.R, inp.b, inp.fn.device)
    return _lib.fn(base, inp.fn.dtype)(*args, _lib.ptr(ws), ws.numel(), outs[4])


_PLAIN_ENTRY = {"auto": "posterior", "generic": "posterior_generic", "rhs": "posterior_rhs"}


def _posterior_call(spec: KernelSpec, inp: _Inputs, gathered: bool, path: str, pq, pn, outs: tuple):
    """(entry point, arguments) of one posterior launch: ``mgp_posterior_gen_*`` for the general-smoothness Matern,
    else by table form -- prepared (``pn`` / ``pq``: the packed neighbour / query tables) or plain, responses in the
    table or gathered.  ``outs``: the pointers of mean, var, ykinvy, info and the stream, in the ABI's order."""
    P = _lib.ptr
    gen = spec.kernel == "matern_gen"
    model = _model_args(spec, inp.ls if pn is None else pn.kernel_length_scale(inp.ls))
    if pn is None and not gen:
        base = "posterior_gathered" if gathered else _PLAIN_ENTRY[path]
        return _lib.fn(base, inp.fn.dtype), _plain_args(inp, model, outs) + outs[4:]
    tail = (inp.mode, inp.eps, P(inp.nz)) + model + outs
    if pn is None:  # (the general smoothness: one entry for both table forms, the absent one NULL)
        tables, shape = (P(inp.fq), P(inp.fn), None, 0, None, 0), (inp.d, P(inp.bi), P(inp.ni), inp.b, inp.k)
    else:
        tables, shape = (P(pq.data), pq.stride, P(pn.data), pn.stride), (pn.d_kernel, P(inp.bi), P(inp.ni), inp.b, inp.k)
    if gen:
        # (`tg` goes along even when the prepared table carries the responses: the library does not read it then)
        tables = tables if pn is None else (None, None) + tables
        return _lib.fn("posterior_gen", inp.fn.dtype), tables + shape + (P(inp.tg), inp.R, int(gathered)) + tail
    if gathered:
        return _lib.fn("posterior_packed_gathered", inp.fn.dtype), tables + shape + (P(inp.tg), inp.R) + tail
    return _lib.fn("posterior_packed", inp.fn.dtype), tables + shape + (inp.R,) + tail


def posterior_mean_var(
    spec: KernelSpec,
    test_features: torch.Tensor,
    train_features: torch.Tensor,
    batch_indices: Optional[torch.Tensor],
    nn_indices: torch.Tensor,
    train_targets: torch.Tensor,
    want_ykinvy: bool = False,
    out_mean: Optional[torch.Tensor] = None,
    out_var: Optional[torch.Tensor] = None,
    info: Optional[torch.Tensor] = None,
    path: str = "auto",
    packed: Union[str, bool] = "auto",
    gathered: bool = False,
):
    """Posterior mean and *unscaled* variance of every batch element, fused.

    Returns ``(mean, var)`` or ``(mean, var, ykinvy)``: mean is ``(b,)`` for 1-D targets
    and ``(b, R)`` for ``(n, R)`` targets (like _muygps_posterior_mean,
    _src/gp/muygps/numpy.py:17-41); var ``(b,)`` equals ``1 - Kcross K^-1 Kcross``
    (:44-67 with Kout = 1); ``ykinvy (b, R)`` holds ``y_r^T K^-1 y_r`` per neighbourhood
    (the summand of _analytic_scale_optim_unnormalized, scale/numpy.py:9-15).

    ``path``: "auto" (dispatcher), or one kernel family by name -- "generic" / "rhs" / "large" (parity tests; the
    general-smoothness Matern has no "rhs").  Which entry points a call tries, in which order: the lists of rungs in
    the body, and the table in DESIGN.md §1.  A closed-form kernel is served up to ``nn_count + 1 + R = 1024`` rows
    (``ValueError`` beyond); the general-smoothness Matern raises :class:`FusedUnsupported` where no fused kernel
    serves it (33 to 64 slots in a batch too small to compile for, more than 1024 rows, a smoothness above 30).
    ``packed``: "auto" reads the tables through prepared copies (:class:`PackedTable`, cached per
    tensor) when the shape allows it and the batch touches the table often enough to pay for the
    one-time pack; True forces, False disables.
    ``gathered``: ``train_targets`` is the already gathered ``(b, k[, R])`` tensor ``targets[nn_indices]``
    (what the reference's ``make_*_tensors`` return) instead of the ``(n[, R])`` table.
    """
    ns = spec.length_scale_batch is not None
    if ns and spec.kernel == "matern_gen":
        raise ValueError("length_scale_batch: the general-smoothness Matern has no per-neighbourhood-scale kernel")
    if ns and path not in ("auto", "generic", "large"):
        raise ValueError(f"length_scale_batch: path is 'auto', 'generic' or 'large', not {path!r}")
    inp = _normalize(spec, test_features, train_features, batch_indices, nn_indices, train_targets, gathered=gathered,
                     per_neighbourhood=ns)
    _debug_check_indices(inp)
    fn, b, R, dtype = inp.fn, inp.b, inp.R, inp.fn.dtype
    mean = out_mean if out_mean is not None else torch.empty((b, R), device=fn.device, dtype=dtype)
    var = out_var if out_var is not None else torch.empty((b,), device=fn.device, dtype=dtype)
    yk = torch.empty((b, R), device=fn.device, dtype=dtype) if want_ykinvy else None
    if path not in ("auto", "generic", "rhs", "large"):
        raise ValueError(f"unknown kernel path {path!r}")
    gen = spec.kernel == "matern_gen"  # one entry point for every table form (mgp_posterior_gen_*)
    if gen and path == "rhs":
        raise ValueError("the general-smoothness Matern goes through the dispatcher (path='auto')")
    if gen and (spec.smoothness is None or not float(spec.smoothness) > 0.0):
        raise ValueError(f"kernel 'matern_gen' needs a positive smoothness, got {spec.smoothness}")
    if gathered and path not in ("auto", "large") and not ((gen or ns) and path == "generic"):
        raise ValueError("gathered responses go through the dispatcher (path='auto') or path='large'")
    # (a separate test table is packed too -- one more pass over ITS rows -- so it counts as table size)
    rows = fn.shape[0] + (0 if test_features is train_features else inp.fq.shape[0])
    # the general smoothness beyond the 64 slots of the wave kernels: the workgroup families, plain tables only
    beyond_wave = gen and inp.k + 1 + R > 64
    use_packed = (path == "auto" and not beyond_wave and not ns
                  and _use_packed(packed, inp, train_features, train_targets, rows, gathered))
    ns_info = torch.zeros(1, device=fn.device, dtype=torch.int32) if ns and info is None else None
    outs = (_lib.ptr(mean), _lib.ptr(var), _lib.ptr(yk), _lib.ptr(info if ns_info is None else ns_info), _lib.stream_ptr())

    def plain():  # the dispatcher on the plain tables, or a closed-form LDS family by name
        call, args = _posterior_call(spec, inp, gathered, path, None, None, outs)
        return call(*args)

    def prepared():
        pn = pack_table(train_features, None if gathered else train_targets, query=False)
        pq = pn if test_features is train_features else pack_table(test_features, None)
        call, args = _posterior_call(spec, inp, gathered, path, pq, pn, outs)
        return call(*args)

    def family(base="posterior_large", slab=True):  # a workgroup family by name, plain tables: on a slab beyond LDS, or in LDS
        return _posterior_plain(base, inp, _model_args(spec, inp.ls), outs, gathered, slab)

    def ns_family(base, slab):  # a length scale per neighbourhood: (b, ls_count) scales, ls_count per row
        model = (spec.kernel_id(), spec.metric_id(), _lib.ptr(inp.ls), inp.ls.shape[1])
        return _posterior_plain(base, inp, model, outs, gathered, slab)

    # the ladders: a rung is tried when the one before it answered MGP_EUNSUPPORTED
    if ns:  # plain tables, the two workgroup families (own info: a bad scale counts there like a bad pivot)
        lds, slab = (lambda: ns_family("posterior_ns_generic", False)), (lambda: ns_family("posterior_ns_large", True))
        rungs = {"auto": (lds, slab), "generic": (lds,), "large": (slab,)}[path]
    elif gen:
        def gen_slab():  # (more than 1024 rows: refused without a call)
            try:
                return family("posterior_gen_large")
            except ValueError:
                return _lib.EUNSUPPORTED

        if path == "generic":
            rungs = (lambda: family("posterior_gen_generic", slab=False),)
        elif path == "large":
            rungs = (gen_slab,)
        elif beyond_wave:
            rungs = (plain, gen_slab)
        else:
            rungs = (prepared if use_packed else plain,)  # (a refusal on the prepared tables is final: the caller's to handle)
    elif path == "large":
        rungs = (family,)
    elif path != "auto":
        rungs = (plain,)
    else:
        rungs = (prepared, plain, family) if use_packed else (plain, family)
    rc, _ = _lib.run_ladder(rungs)
    if gen and rc == _lib.EUNSUPPORTED:
        raise FusedUnsupported(f"general-smoothness Matern: no fused kernel for {dtype}, k={inp.k}, R={R}, d={inp.d}")
    _lib.check(rc, "mgp_posterior_ns" if ns else "mgp_posterior_gen" if gen else "mgp_posterior")
    if ns_info is not None and b > 0:
        # the counter this call owns (a caller that passes ``info=`` looks at its own, as on the scalar path): a
        # non-positive or non-finite scale counts there like a non-positive pivot
        _lib.raise_if_not_spd(ns_info, NS_NOT_SPD)
    mean_out = mean.reshape(b) if inp.squeeze else mean.reshape(b, R)
    if want_ykinvy:
        return mean_out, var, (yk.reshape(b) if inp.squeeze else yk)
    return mean_out, var


def _loocv_call(table, inp: _Inputs, spec: KernelSpec, ls: torch.Tensor, *, eps, mean, var, yk, info, huber_delta: float,
                partials, scratch, stream):
    """(entry point, arguments) of one LOOCV evaluation: ``mgp_loocv_packed_*`` on the prepared ``table``, or
    ``mgp_loocv_*`` on the plain tables (``table`` None).  ``ls``: the length scale(s) the kernel reads -- padded to the
    table's ``d_kernel`` by the caller; ``eps``: a float, or the ctypes double a prepared evaluation updates in place."""
    P = _lib.ptr
    if table is not None:
        base, head = "loocv_packed", (P(table.data), table.stride, table.d_kernel, P(inp.bi), P(inp.ni), inp.b, inp.k)
    else:
        base, head = "loocv", (P(inp.fn), inp.d, P(inp.bi), P(inp.ni), inp.b, inp.k, P(inp.tg))
    args = head + (inp.mode, eps, P(inp.nz), spec.kernel_id(), spec.metric_id(), P(ls), ls.numel(), P(mean), P(var), P(yk),
                   P(info), float(huber_delta), P(partials), P(scratch), stream)
    return _lib.fn(base, inp.fn.dtype), args


def loocv_partials(
    spec: KernelSpec,
    train_features: torch.Tensor,
    train_targets: torch.Tensor,
    batch_indices: torch.Tensor,
    nn_indices: torch.Tensor,
    huber_delta: float = 1.5,
    packed: Union[str, bool] = "auto",
    info: Optional[torch.Tensor] = None,
    return_ykinvy: bool = False,
):
    """One shard's LOOCV evaluation in one library call (``mgp_loocv_*``): the fused launch over
    the training table on both sides, then the six fp64 partial sums
    ``[sum r^2/v, sum log v, sum r^2, b, sum pseudo-Huber, sum y^T K^-1 y]`` the losses
    (_src/optimize/loss/numpy.py:22-61) and the analytic scale (scale/numpy.py:11-18) are built
    from -- no host work between the two.  Returns ``(partials float64 (6,), mean (b,), var (b,))``,
    all on the device.  One response."""
    inp = _normalize(spec, train_features, train_features, batch_indices, nn_indices, train_targets, responses="single")
    _debug_check_indices(inp)
    fn, b, dtype = inp.fn, inp.b, inp.fn.dtype
    mean = torch.empty((b,), device=fn.device, dtype=dtype)
    var = torch.empty((b,), device=fn.device, dtype=dtype)
    yk = torch.empty((b,), device=fn.device, dtype=dtype)
    partials = torch.empty(6, device=fn.device, dtype=torch.float64)
    scratch, stream = _lib.loocv_scratch(fn.device, b), _lib.stream_ptr()

    def plain(table=None):  # mgp_loocv_packed_* on a prepared table, mgp_loocv_* on the plain one
        ls = inp.ls if table is None else table.kernel_length_scale(inp.ls)
        call, args = _loocv_call(table, inp, spec, ls, eps=inp.eps, mean=mean, var=var, yk=yk, info=info,
                                 huber_delta=huber_delta, partials=partials, scratch=scratch, stream=stream)
        return call(*args)

    def prepared():
        return plain(pack_table(train_features, train_targets))

    def slab():  # a system beyond LDS: the blocked factorisation in global memory (closed-form kernels)
        outs = (_lib.ptr(mean), _lib.ptr(var), _lib.ptr(yk), _lib.ptr(info), _lib.stream_ptr())
        return _posterior_plain("posterior_large", inp, _model_args(spec, inp.ls), outs, False, slab=True)

    rungs = (prepared,) if _use_packed(packed, inp, train_features, train_targets, fn.shape[0]) else ()
    rungs += (plain,) if spec.kernel == "matern_gen" else (plain, slab)
    rc, at = _lib.run_ladder(rungs)
    if rungs[at] is slab:
        # ... then the same reduction tree over its outputs on the canonical leaves (what mgp_loocv_* does behind every
        # kernel family but the wave kernels)
        _lib.check(rc, "mgp_posterior_large")
        partials = loocv_tree_sums(mean, var, yk, inp.tg, inp.bi, huber_delta)
    if rc != 0:
        _lib.loocv_scratch_reset()
    _lib.check(rc, "mgp_loocv")
    if return_ykinvy:
        return partials, mean, var, yk
    return partials, mean, var


class LoocvPlan:
    """A prepared LOOCV objective evaluation: everything that does not change between the evaluations of a
    hyper-parameter search -- prepared table, index tensors, output and scratch buffers, the bound C entry point with its
    argument list -- is set up once; :meth:`launch` then costs one ctypes call (= one kernel launch: the fused kernel
    walks the reduction tree itself) and :meth:`wait` reads the six partial sums from PINNED HOST memory the kernel wrote
    them to, by polling: no stream synchronisation, no device-to-host copy.  What an optimiser's loop pays per evaluation
    drops from ~55 us of host work around a 215 us kernel (config 3's strong-scaling shard, 125 k neighbourhoods) to ~10.

    Reference semantics: one call of the objective ``obj_fn(**hyper)`` of ``make_loo_crossval_fn``
    (optimize/objective.py:20-105) up to the partial sums ``[sum r^2/v, sum log v, sum r^2, b, sum pseudo-Huber,
    sum y^T K^-1 y]`` (``distributed.finish_objective`` turns them into sigma^2 and the loss).

    ``length_scale`` per evaluation: a float (Isotropy) or a sequence of d floats (Anisotropy: copied to the device by
    one asynchronous transfer); ``noise``: a float (HomoscedasticNoise), or fixed per plan as a tensor (heteroscedastic
    table ``(n,)`` / batch ``(b, k)``).  One response.

    The length scale of Isotropy and the result slot are single words of pinned host memory the kernel reads /
    writes while it runs, so ONE evaluation is in flight per plan: :meth:`launch` waits for the previous one if the
    caller did not (``wait()``, or -- device-side partials -- whatever consumed them), and it must be called under the
    stream the plan was made on.  ``info`` (the kernels' count of non-positive pivots) is looked at when a sum comes
    back NaN: ``numpy.linalg.LinAlgError`` as everywhere else (``config.state.check_spd``)."""

    def __init__(self, kernel: str, metric: str, train_features: torch.Tensor, train_targets: torch.Tensor,
                 batch_indices: torch.Tensor, nn_indices: torch.Tensor, anisotropic: bool = False,
                 noise_tensor: Optional[torch.Tensor] = None, huber_delta: float = 1.5, packed: Union[str, bool] = "auto",
                 host_result: bool = True):
        import numpy as np

        _lib.require_cuda(train_features, train_targets, batch_indices, nn_indices, noise_tensor)
        _lib.loocv_tree_selfcheck(train_features.device)  # (once per process: in-kernel walk vs the walk by kernels)
        self.spec = KernelSpec(kernel, metric, 1.0, 0.0)
        # (the noise mode and table are fixed per plan; the length scale is the plan's own buffer below)
        inp = _normalize(KernelSpec(kernel, metric, 1.0, 0.0 if noise_tensor is None else noise_tensor), train_features,
                         train_features, batch_indices, nn_indices, train_targets, responses="single")
        fn, dtype, dev = inp.fn, inp.fn.dtype, inp.fn.device
        self.d, self.b, self.k, self.ni, self.bi = inp.d, inp.b, inp.k, inp.ni, inp.bi
        b = inp.b
        self.dtype, self.device, self.anisotropic = dtype, dev, bool(anisotropic)
        self._keep = (train_features, train_targets, batch_indices, nn_indices, fn, inp.tg, noise_tensor)
        self._nz = inp.nz
        self.mean = torch.empty((b,), device=dev, dtype=dtype)
        self.var = torch.empty((b,), device=dev, dtype=dtype)
        self.ykinvy = torch.empty((b,), device=dev, dtype=dtype)
        self.info = torch.zeros(1, device=dev, dtype=torch.int32)
        self.scratch = torch.zeros(int(_lib.load().mgp_loocv_scratch_bytes()), dtype=torch.uint8, device=dev)
        # the six sums: pinned host memory the kernel writes directly (mapped into the device's address space), or a
        # device tensor (a sharded evaluation all-reduces them on the device first)
        self.host_result = bool(host_result) and b > 0
        if self.host_result:
            self._res_t = torch.zeros(8, dtype=torch.float64).pin_memory()
            self._res = self._res_t.numpy()
            self.partials = self._res_t
        else:
            self.partials = torch.zeros(6, device=dev, dtype=torch.float64)
        use_packed = _use_packed(packed, inp, train_features, train_targets, fn.shape[0], threshold=False)
        self._table = pack_table(train_features, train_targets) if use_packed else None
        dk = self._table.d_kernel if use_packed else inp.d
        # length scales: Isotropy -- one value in pinned host memory, read once per workgroup; Anisotropy -- the kernels
        # read them per task: a device buffer refreshed by an asynchronous copy from pinned memory
        self._ls_host = torch.ones(dk if anisotropic else 1, dtype=dtype).pin_memory()
        self._ls_np = self._ls_host.numpy()
        self._ls_dev = torch.ones(dk, device=dev, dtype=dtype) if anisotropic else None
        self._eps = _lib.C.c_double(0.0)  # (the one argument that changes per evaluation: set in place)
        # (every argument converted once: an evaluation is one foreign call on ready-made objects; the stream is the
        # one current when the plan was made -- the plan's scratch must not serve two streams anyway)
        self._stream = _lib.stream_ptr()
        self._raw_stream = _lib.raw_stream()
        self._in_flight = None  # an event behind the last launch whose completion nobody has observed yet
        self._fn, args = _loocv_call(self._table, inp, self.spec, self._ls_dev if anisotropic else self._ls_host,
                                     eps=self._eps, mean=self.mean, var=self.var, yk=self.ykinvy, info=self.info,
                                     huber_delta=huber_delta, partials=self.partials, scratch=self.scratch,
                                     stream=self._stream)
        self._args = tuple(a if isinstance(a, _lib.C._SimpleCData) or a is None else t(a) for a, t in zip(args, self._fn.argtypes))
        self._np = np
        self._launched = False

    def launch(self, length_scale, noise: float = 0.0) -> None:
        """Put one evaluation on the plan's stream (nothing waits, unless the previous evaluation is still running)."""
        if _lib.raw_stream() != self._raw_stream:
            raise RuntimeError("LoocvPlan.launch(): the current stream is not the one the plan was prepared on")
        if self._in_flight is not None:
            # the kernel in flight reads the length-scale word and writes the result slot this call is about to reset
            if self.host_result:
                self.wait()
            else:
                self._in_flight.synchronize()
            self._in_flight = None
        if self.anisotropic:
            ls = self._np.asarray(length_scale, dtype=self._ls_np.dtype).reshape(-1)
            if ls.size != self.d:
                raise ValueError(f"Difference tensor of shape (..., {self.d}) must have final dimension size of {ls.size}")
            self._ls_np[: self.d] = ls
            self._ls_dev.copy_(self._ls_host, non_blocking=True)
        else:
            self._ls_np[0] = length_scale
        self._eps.value = noise
        if self.host_result:
            self._res[3] = 0.0  # (the kernel writes the count last)
        rc = self._fn(*self._args)
        if rc != 0:
            self.scratch.zero_()
        _lib.check(rc, "mgp_loocv")
        self._launched = True
        if self.host_result:
            self._in_flight = True
        elif self.b > 0:
            self._in_flight = torch.cuda.Event()
            self._in_flight.record()

    def _check_spd(self, sums) -> None:
        if sums[0] != sums[0] or sums[1] != sums[1] or sums[5] != sums[5]:  # NaN: some neighbourhood did not factorise
            from muygpys_amd.config import config

            bad = int(self.info.item())
            self.info.zero_()
            if bad and config.state.check_spd:
                _lib._raise_not_spd(bad, "LOOCV evaluation")

    def wait(self, spin_seconds: float = 2.0):
        """The six partial sums of the evaluation last launched, as host floats (numpy float64 array)."""
        if not self._launched:
            raise RuntimeError("LoocvPlan.wait() before launch()")
        if self.b == 0:
            return self._np.zeros(6)
        if not self.host_result:
            sums = self.partials.cpu().numpy()
            self._in_flight = None
            self._check_spd(sums)
            return sums
        import time

        res, want = self._res, float(self.b)
        deadline = None
        while res[3] != want:
            if deadline is None:
                deadline = time.perf_counter() + spin_seconds
            elif time.perf_counter() > deadline:  # (never in a healthy run: fall back to the stream's own completion)
                torch.cuda.current_stream().synchronize()
                if res[3] != want:
                    raise _lib.HipLibraryError("mgp_loocv: the kernel finished without publishing its sums")
        self._in_flight = None
        sums = res[:6].copy()
        self._check_spd(sums)
        return sums

    def evaluate(self, length_scale, noise: float = 0.0):
        self.launch(length_scale, noise)
        return self.wait()



def _hyper_partials(spec: KernelSpec, inp: _Inputs, info, gm, gv, gyk=None, want_noise: bool = True, want_nu: bool = False):
    """One backward launch for the hyper-parameters: the per-neighbourhood partials ``(g_l (b, ls_count), g_n (b, k) or
    None)`` of the cotangents ``gm`` / ``gv`` (either may be None) -- and ``gyk`` of ``y^T K^-1 y``: given, the launch is
    the LOOCV objective's (``mgp_loocv_backward_*``, one response), else ``mgp_posterior_backward_*`` with no feature or
    response cotangents.  The noise is ``spec``'s (homoscedastic); everything else comes from ``inp``.

    A closed-form kernel whose two triangles no longer fit LDS (``nn_count`` beyond ``mgp_max_nn_count_backward``) goes
    to the backward on the slab factor (``mgp_hyper_backward_large_*``, csrc/mgp_backward_large.hip), up to
    ``mgp_large_max_nn_count(elem_size, 1)`` = 1022 whatever the response count; ``ValueError`` beyond.

    The general-smoothness Matern has its own backward on the slab factor at every ``nn_count``
    (``mgp_hyper_backward_gen_large_*``, csrc/mgp_backward_gen_large.hip) with ``spec.smoothness``, up to
    ``mgp_backward_gen_large_max_nn_count``; ``ValueError`` beyond -- and, on request (:func:`gen_backward`), the LDS
    workgroup backward ``mgp_posterior_backward_gen_*`` in front of it where that one is faster.  ``want_nu`` (that kernel alone): a third result,
    the per-neighbourhood partials ``g_nu (b,)`` with respect to the smoothness."""
    P = _lib.ptr
    fn, ls = inp.fn, inp.ls
    if spec.kernel == "matern_gen":
        return _hyper_partials_gen(spec, inp, info, gm, gv, gyk, want_noise, want_nu)
    if want_nu:
        raise ValueError(f"kernel {spec.kernel!r} has a fixed smoothness: no gradient with respect to it")
    g_l = torch.zeros((inp.b, ls.numel()), device=fn.device, dtype=fn.dtype)
    g_n = torch.zeros((inp.b, inp.k), device=fn.device, dtype=fn.dtype) if want_noise else None
    gm, gv = (None if g is None else g.contiguous() for g in (gm, gv))
    model = (_lib.NOISE_SCALAR, float(spec.noise), None, spec.kernel_id(), spec.metric_id(), P(ls), ls.numel())
    shape = (inp.d, P(inp.bi), P(inp.ni), inp.b, inp.k, P(inp.tg))
    out = (P(g_l), P(g_n), P(info))
    what = ("mgp_posterior_backward" if gyk is None else "mgp_loocv_backward", "mgp_hyper_backward_large")

    def lds():
        if gyk is not None:
            return _lib.fn("loocv_backward", fn.dtype)(P(fn), *shape, *model, P(gm), P(gv), P(gyk), *out, _lib.stream_ptr())
        return _lib.fn("posterior_backward", fn.dtype)(P(fn), P(fn), *shape, inp.R, *model, P(gm), P(gv), None, None, None,
                                                       *out, _lib.stream_ptr())

    def slab():
        ws = _lib.backward_large_workspace(fn.dtype, inp.k, inp.b, fn.device)
        return _lib.fn("hyper_backward_large", fn.dtype)(P(fn), *shape, inp.R, *model, P(gm), P(gv), P(gyk), *out,
                                                         P(ws), ws.numel(), _lib.stream_ptr())

    rc, at = _lib.run_ladder((lds,) if spec.kernel == "matern_gen" else (lds, slab))
    _lib.check(rc, what[at])
    return g_l, g_n


# which rung serves the hyper-parameter partials of the general-smoothness Matern first: "slab" (the backward on the slab
# factor alone, csrc/mgp_backward_gen_large.hip) or "lds" (the LDS workgroup backward, csrc/mgp_backward_gen.hip, with
# the slab behind it for an nn_count beyond mgp_max_nn_count_backward_gen).  MUYGPYS_HIP_GEN_BACKWARD, unset = slab.
GEN_BACKWARD_MODES = ("slab", "lds")
# ... and the largest nn_count at which the "lds" rung is tried, by element size: where it was measured to beat the slab
# backward (profiles/gen_backward_lds_bench.json, d = 40, 200 000 neighbourhoods, nu = 1.3: fp32 4.0x at nn_count 30 and
# 2.1x at 63, 0.77x at 100; fp64 2.5x at 30, 0.72x at 63 -- one 128-thread workgroup per CU there).  Nothing was
# measured between those shapes: the rung ends at the last one it won.
GEN_BACKWARD_LDS_MAX_NN_COUNT = {4: 63, 8: 30}


def _gen_backward_from_env() -> str:
    mode = os.environ.get("MUYGPYS_HIP_GEN_BACKWARD", "") or "slab"
    if mode not in GEN_BACKWARD_MODES:
        raise ValueError(f"MUYGPYS_HIP_GEN_BACKWARD={mode!r} is none of {GEN_BACKWARD_MODES}")
    return mode


_GEN_BACKWARD = _gen_backward_from_env()


@contextlib.contextmanager
def gen_backward(mode: str):
    """``with fused.gen_backward("lds"):`` -- the first rung of the general-smoothness Matern's analytic gradients inside
    the block (:func:`loocv_value_and_grad`, :func:`class_value_and_grad` and the optimisers on top of them); the
    previous mode is restored on the way out."""
    global _GEN_BACKWARD
    if mode not in GEN_BACKWARD_MODES:
        raise ValueError(f"gen_backward mode {mode!r} is none of {GEN_BACKWARD_MODES}")
    previous, _GEN_BACKWARD = _GEN_BACKWARD, mode
    try:
        yield
    finally:
        _GEN_BACKWARD = previous


def gen_backward_default() -> str:
    """The mode in force right now (the environment's choice, or an enclosing block's)."""
    return _GEN_BACKWARD


# how the fast-posterior-mean workflow serves the general-smoothness Matern: "materialised" (coefficients through
# mgp_pairwise_dists_* + mgp_matern_gen_* + mgp_solve_* in row chunks, predictions through a materialised Kcross and an
# einsum) or "fused" (one mgp_fast_coefficients_gen_* launch for the table, one mgp_fast_posterior_mean_gen_* launch per
# query batch; the materialised route behind them where the library refuses: nu > 30, more than 1024 rows).
# MUYGPYS_HIP_GEN_FAST, unset = materialised.
GEN_FAST_MODES = ("materialised", "fused")


def _gen_fast_from_env() -> str:
    mode = os.environ.get("MUYGPYS_HIP_GEN_FAST", "") or "materialised"
    if mode not in GEN_FAST_MODES:
        raise ValueError(f"MUYGPYS_HIP_GEN_FAST={mode!r} is none of {GEN_FAST_MODES}")
    return mode


_GEN_FAST = _gen_fast_from_env()


@contextlib.contextmanager
def gen_fast(mode: str):
    """``with fused.gen_fast("fused"):`` -- the general-smoothness Matern on the fused coefficient and prediction kernels
    inside the block (:func:`fast_coefficients`, :func:`fast_posterior_mean`, ``lazy_eval.fast_mean`` and the example
    workflow on top of them); the previous mode is restored on the way out."""
    global _GEN_FAST
    if mode not in GEN_FAST_MODES:
        raise ValueError(f"gen_fast mode {mode!r} is none of {GEN_FAST_MODES}")
    previous, _GEN_FAST = _GEN_FAST, mode
    try:
        yield
    finally:
        _GEN_FAST = previous


def gen_fast_default() -> str:
    """The mode in force right now (the environment's choice, or an enclosing block's)."""
    return _GEN_FAST


def _gen_smoothness(spec: KernelSpec) -> float:
    """nu of a general-smoothness model; the forward's ``ValueError`` for a missing or non-positive one."""
    if spec.smoothness is None or not float(spec.smoothness) > 0.0:
        raise ValueError(f"kernel 'matern_gen' needs a positive smoothness, got {spec.smoothness}")
    return float(spec.smoothness)


def _hyper_partials_gen(spec: KernelSpec, inp: _Inputs, info, gm, gv, gyk, want_noise: bool, want_nu: bool):
    """:func:`_hyper_partials` of the general-smoothness Matern: ``(g_l, g_n or None[, g_nu])``.  The ladder is the
    slab backward alone, or -- :func:`gen_backward` ``"lds"``, up to ``GEN_BACKWARD_LDS_MAX_NN_COUNT`` --
    ``mgp_posterior_backward_gen_*`` with the slab behind it."""
    P = _lib.ptr
    fn, ls = inp.fn, inp.ls
    nu = spec.smoothness
    if nu is None or not float(nu) > 0.0:
        raise ValueError(f"kernel 'matern_gen' needs a positive smoothness, got {nu}")
    limit = int(_lib.load().mgp_backward_gen_large_max_nn_count(fn.element_size()))
    if inp.k > limit:
        raise ValueError(f"analytic gradients of the general-smoothness Matern: nn_count = {inp.k} is beyond "
                         f"mgp_backward_gen_large_max_nn_count = {limit}")
    g_l = torch.zeros((inp.b, ls.numel()), device=fn.device, dtype=fn.dtype)
    g_n = torch.zeros((inp.b, inp.k), device=fn.device, dtype=fn.dtype) if want_noise else None
    g_nu = torch.zeros((inp.b,), device=fn.device, dtype=fn.dtype) if want_nu else None
    gm, gv = (None if g is None else g.contiguous() for g in (gm, gv))
    shape = (inp.d, P(inp.bi), P(inp.ni), inp.b, inp.k, P(inp.tg), inp.R)
    model = (_lib.NOISE_SCALAR, float(spec.noise), None, float(nu), spec.metric_id(), P(ls), ls.numel())
    cotangents = (P(gm), P(gv), P(gyk))

    def lds():  # (the training table on both sides, no feature or response cotangents)
        return _lib.fn("posterior_backward_gen", fn.dtype)(
            P(fn), P(fn), *shape, *model, *cotangents, None, None, None, P(g_l), P(g_n), P(g_nu), P(info), _lib.stream_ptr())

    def slab():
        ws = _lib.backward_large_workspace(fn.dtype, inp.k, inp.b, fn.device)
        return _lib.fn("hyper_backward_gen_large", fn.dtype)(
            P(fn), *shape, *model, *cotangents, P(g_l), P(g_n), P(g_nu), P(info), P(ws), ws.numel(), _lib.stream_ptr())

    use_lds = _GEN_BACKWARD == "lds" and inp.k <= GEN_BACKWARD_LDS_MAX_NN_COUNT[fn.element_size()]
    rungs = ((lds, "mgp_posterior_backward_gen"),) if use_lds else ()
    rungs += ((slab, "mgp_hyper_backward_gen_large"),)
    rc, at = _lib.run_ladder([r for r, _ in rungs])
    _lib.check(rc, rungs[at][1])
    return (g_l, g_n, g_nu) if want_nu else (g_l, g_n)


def _hyper_gradient(g_l, g_n, info, what: str, reduce_fn, g_nu=None):
    """The tail of an analytic gradient: the SPD check of the backward launches, deterministic fp64 column sums of
    their partials, the sum over the ranks -- ``(grad_length_scale (numpy, ls_count), grad_noise (float))``, and
    ``grad_smoothness (float)`` behind them when ``g_nu`` is given."""
    import numpy as np

    _lib.raise_if_not_spd(info, what)
    cols = [_lib.column_sums(g_l), _lib.column_sums(g_n.reshape(-1, 1))]  # fp64, deterministic
    if g_nu is not None:
        cols.append(_lib.column_sums(g_nu.reshape(-1, 1)))
    grad = torch.cat(cols)
    if reduce_fn is not None:
        reduce_fn(grad)
    g = grad.cpu().numpy()
    if g_nu is not None:
        return np.asarray(g[:-2], dtype=np.float64), float(g[-2]), float(g[-1])
    return np.asarray(g[:-1], dtype=np.float64), float(g[-1])


def _loocv_forward(spec: KernelSpec, train_features, train_targets, bi, ni, packed, huber_delta: float):
    """``(partials, mean, var, ykinvy)`` of one LOOCV evaluation: :func:`loocv_partials`, or -- the general-smoothness
    Matern, which ``mgp_loocv_*`` serves on the wave kernels alone -- the fused posterior with ``y^T K^-1 y`` at any
    ``nn_count`` followed by the reduction tree over its outputs (:func:`loocv_tree_sums`)."""
    if spec.kernel != "matern_gen":
        return loocv_partials(spec, train_features, train_targets, bi, ni, packed=packed, return_ykinvy=True,
                              huber_delta=huber_delta)
    mean, var, yk = posterior_mean_var(spec, train_features, train_features, bi, ni, train_targets, want_ykinvy=True,
                                       packed=packed)
    mean, var, yk = mean.reshape(-1), var.reshape(-1), yk.reshape(-1)
    return loocv_tree_sums(mean, var, yk, train_targets, bi, huber_delta), mean, var, yk


def loocv_value_and_grad(spec: KernelSpec, train_features: torch.Tensor, train_targets: torch.Tensor,
                         batch_indices: torch.Tensor, nn_indices: torch.Tensor, loss: str = "lool",
                         packed: Union[str, bool] = "auto", reduce_fn=None, scale=("analytic", 1),
                         boundary_scale: Optional[float] = None, sigma_noise: Optional[float] = None,
                         grad_smoothness: bool = False):
    """A LOOCV loss and its ANALYTIC gradient with respect to the length scale(s) and a homoscedastic noise: one
    forward evaluation (``mgp_loocv_*``) and one backward launch (``mgp_loocv_backward_*``) instead of the ``p + 1``
    forward evaluations per iteration scipy's finite differences cost the reference's L-BFGS-B driver
    (_src/optimize/chassis/numpy.py:57-81).  The reference gets such gradients from torch autograd over its torch
    backend (torch/muygps_layer.py:129-164); here the chain rule is written out.  With r = mean - y, v the unscaled
    variance, s = sigma^2 and (reference: _src/optimize/loss/numpy.py:22-117)

        lool          sum r^2 / (s v) + log(s v)            d/dm = 2 r / (s v)   d/dv = 1/v - r^2 / (s v^2)   d/ds = sum 1/s - r^2 / (s^2 v)
        mse           sum r^2 / n                           d/dm = 2 r / n
        pseudo_huber  d^2 sum sqrt(1 + (r/d)^2) - 1         d/dm = r / sqrt(1 + (r/d)^2)
        looph         sum 2 d^2 (g - 1) + log(s v),         d/dm = 2 r / (g s v)   d/dv = 1/v - r^2 / (g s v^2)   d/ds = sum 1/s - r^2 / (g s^2 v)
                      g = sqrt(1 + r^2 / (d^2 s v))

    (d = ``boundary_scale``: 1.5 / 3.0 by default, as in the reference), sigma^2 enters through
    ``d s / d (y_i^T K_i^-1 y_i) = (ds / df0) / (n k)`` -- the analytic scale, scale/numpy.py:18-34 -- and the
    backward kernel turns the three cotangents into per-neighbourhood partials of d / d length_scale and d / d noise.
    ``reduce_fn`` (sharded batches): sums a float64 device vector over the ranks in place -- applied to every sum the
    cotangents are formed from and to the gradient.

    ``scale`` names the sigma^2: ``("analytic", iteration_count)`` -- the closed form, followed by
    ``iteration_count - 1`` passes of ``s <- (s + f0 / s) / 2`` on the first value ``f0`` (gp/hyperparameter/scale.py:
    205-217 of the reference; ``ds / df0`` by the same recurrence) -- or ``("fixed", value)``: a constant, nothing
    flows through ``y^T K^-1 y`` (``FixedScale``, the reference's ``noop_scale_opt_fn``).

    ``sigma_noise``: the noise inside sigma^2 when it is NOT ``spec.noise`` -- the reference's objective evaluates mean
    and variance at the TRIAL noise of the optimiser but the analytic scale at the model's STORED one
    (gp/hyperparameter/scale.py:206,214 against gp/noise/homoscedastic.py:112-113).  Then ``y^T K^-1 y`` comes from a
    second forward launch at ``sigma_noise`` and its cotangent goes back through a second backward launch there; the
    returned noise gradient is the trial noise's (sigma^2 does not depend on it).

    Any ``nn_count`` the forward serves: beyond ``mgp_max_nn_count_backward`` the backward launches run on the slab
    factor in global memory (``mgp_hyper_backward_large_*``), up to ``nn_count = 1022``; ``ValueError`` beyond.

    The general-smoothness Matern (``spec.kernel == "matern_gen"``): the forward is the fused posterior with
    ``y^T K^-1 y`` and the reduction tree over its outputs, the backward ``mgp_hyper_backward_gen_large_*`` at every
    ``nn_count`` up to 1022.  ``grad_smoothness`` (that kernel alone): the gradient with respect to nu as well -- the
    cotangent of ``y^T K^-1 y`` (the analytic sigma^2 with its fixed-point passes, the ``sigma_noise`` split with its
    second backward launch) reaches it the way it reaches the length scales.

    Returns ``(value, grad_length_scale (numpy, ls_count), grad_noise (float))`` of the LOSS (the objective the
    drivers maximise is its negative); with ``grad_smoothness`` ``(value, grad_ls, grad_noise, grad_nu (float))``."""
    import copy
    import math

    if loss not in ("lool", "mse", "pseudo_huber", "looph"):
        raise NotImplementedError(f"analytic gradients are written out for lool, mse, pseudo_huber and looph, not {loss!r}")
    if isinstance(spec.noise, torch.Tensor) and spec.noise.ndim >= 1:
        raise NotImplementedError("analytic gradients: homoscedastic noise")
    if grad_smoothness and spec.kernel != "matern_gen":
        raise ValueError(f"grad_smoothness: kernel {spec.kernel!r} has a fixed smoothness")
    inp = _normalize(spec, train_features, train_features, batch_indices, nn_indices, train_targets, responses="single")
    dtype, tg, ni, bi, k = inp.fn.dtype, inp.tg, inp.ni, inp.bi, inp.k
    needs_scale = loss in ("lool", "looph")
    delta = float(boundary_scale) if boundary_scale is not None else (3.0 if loss == "looph" else 1.5)
    huber = delta if loss == "pseudo_huber" else 1.5
    partials, mean, var, yk = _loocv_forward(spec, train_features, train_targets, bi, ni, packed, huber)
    # (sigma_noise given = the noise is a VARIABLE of the caller's function while sigma^2 holds its own, constant one:
    # the cotangent of y^T K^-1 y must not reach the noise gradient even where the two values coincide)
    split_bwd = needs_scale and scale[0] == "analytic" and sigma_noise is not None
    split = split_bwd and float(sigma_noise) != float(spec.noise)
    spec_s = spec
    if split:  # sigma^2 at the stored noise: y^T K^-1 y of a second evaluation
        spec_s = copy.copy(spec)
        spec_s.noise = float(sigma_noise)
        partials_s = _loocv_forward(spec_s, train_features, train_targets, bi, ni, packed, 1.5)[0]
        partials = torch.cat([partials[:5], partials_s[5:6]])
    if reduce_fn is not None:
        reduce_fn(partials)
    A, B, r2sum, n, ph, cy = (float(v) for v in partials.tolist())
    mode, arg = scale
    if mode == "analytic":
        s = f0 = cy / (n * k)
        ds = 1.0                                  # d s / d f0 through the fixed-point passes
        for _ in range(1, int(arg)):
            s, ds = 0.5 * (s + f0 / s), 0.5 * (ds + 1.0 / s - f0 * ds / (s * s))
    elif mode == "fixed":
        s, ds = float(arg), 0.0
    else:
        raise ValueError(f"scale = {scale!r}: ('analytic', iteration_count) or ('fixed', value)")
    r = mean - tg[:, 0][bi]
    dL_ds = 0.0
    gv = None
    if loss == "lool":
        value = A / s + B + n * math.log(s)
        gm = (2.0 / s) * r / var
        gv = 1.0 / var - (r * r) / (s * var * var)
        dL_ds = n / s - A / (s * s)
    elif loss == "mse":
        value = r2sum / n
        gm = (2.0 / n) * r
    elif loss == "pseudo_huber":
        value = ph
        gm = r / torch.sqrt(1.0 + (r / delta) ** 2)
    else:  # looph: not separable in sigma^2 -- its sums are formed here, in fp64, once sigma^2 is known
        r64, v64 = r.double(), var.double()
        g = torch.sqrt(1.0 + r64 * r64 / (delta * delta * s * v64))
        sums = torch.stack([(2.0 * delta * delta * (g - 1.0) + torch.log(s * v64)).sum(), (r64 * r64 / (g * v64)).sum()])
        if reduce_fn is not None:
            reduce_fn(sums)
        value, rgv = (float(x) for x in sums.tolist())
        gm = (2.0 * r64 / (g * s * v64)).to(dtype)
        gv = (1.0 / v64 - r64 * r64 / (g * s * v64 * v64)).to(dtype)
        dL_ds = n / s - rgv / (s * s)
    zeros = torch.zeros_like(var)
    gv = zeros if gv is None else gv
    gyk_value = dL_ds * ds / (n * k) if needs_scale else 0.0
    info = torch.zeros(1, device=inp.fn.device, dtype=torch.int32)
    nu = {"want_nu": True} if grad_smoothness else {}
    if split_bwd:
        g_l, g_n, *g_nu = _hyper_partials(spec, inp, info, gm, gv, zeros, **nu)
        second = _hyper_partials(spec_s, inp, info, zeros, zeros, torch.full_like(var, gyk_value), want_noise=False, **nu)
        g_l = g_l + second[0]
        g_nu = [g_nu[0] + second[2]] if grad_smoothness else g_nu
    else:
        g_l, g_n, *g_nu = _hyper_partials(spec, inp, info, gm, gv,
                                          torch.full_like(var, gyk_value) if gyk_value != 0.0 else zeros, **nu)
    return (value, *_hyper_gradient(g_l, g_n, info, "LOOCV gradient", reduce_fn, *g_nu))


def class_value_and_grad(spec: KernelSpec, train_features: torch.Tensor, train_labels: torch.Tensor,
                         batch_indices: torch.Tensor, nn_indices: torch.Tensor, loss: str = "cross_entropy",
                         packed: Union[str, bool] = "auto", reduce_fn=None, grad_smoothness: bool = False):
    """A classification LOOCV loss on ``R >= 2`` one-hot response columns and its ANALYTIC gradient with respect to
    the length scale(s) and a homoscedastic noise: the fused posterior (``posterior_mean_var``), one
    ``mgp_class_sums_*`` launch that returns the loss sums and the cotangent of the (b, R) mean, and one
    ``mgp_posterior_backward_*`` launch fed with that cotangent (``grad_var`` = NULL: neither loss reads the variance,
    so no sigma^2 enters and the trial / stored noise split of :func:`loocv_value_and_grad` does not arise).

        cross_entropy  -sum one_hot log clip(softmax(mean))      (reference: _src/optimize/loss/numpy.py:12-19)
        mse            sum r^2 / (b R),  d/dm = 2 r / (b R)       (:22-31, ``np.prod(predictions.shape)``)

    ``reduce_fn`` (sharded batches): sums a float64 device vector over the ranks in place -- applied to the sums (so
    the mse count is the global one) and to the gradient.

    Any ``nn_count`` the forward serves (``nn_count + 1 + R <= 1024``): beyond ``mgp_max_nn_count_backward`` the
    backward launch runs on the slab factor in global memory (``mgp_hyper_backward_large_*``).  The general-smoothness
    Matern: ``mgp_hyper_backward_gen_large_*`` at every ``nn_count`` up to 1022, and with ``grad_smoothness`` the gradient
    with respect to nu as a fourth result.

    Returns ``(value, grad_length_scale (numpy, ls_count), grad_noise (float))`` of the LOSS."""
    if loss not in ("cross_entropy", "mse"):
        raise NotImplementedError(f"classification gradients are written out for cross_entropy and mse, not {loss!r}")
    if isinstance(spec.noise, torch.Tensor) and spec.noise.ndim >= 1:
        raise NotImplementedError("analytic gradients: homoscedastic noise")
    if grad_smoothness and spec.kernel != "matern_gen":
        raise ValueError(f"grad_smoothness: kernel {spec.kernel!r} has a fixed smoothness")
    inp = _normalize(spec, train_features, train_features, batch_indices, nn_indices, train_labels, responses="labels")
    fn, tg, bi, b, R = inp.fn, inp.tg, inp.bi, inp.b, inp.R
    info = torch.zeros(1, device=fn.device, dtype=torch.int32)
    mean, _ = posterior_mean_var(spec, fn, fn, bi, inp.ni, tg, info=info, packed=packed)
    _lib.raise_if_not_spd(info, "classification objective")
    stride = R * tg.element_size()
    if loss == "mse" and reduce_fn is not None:  # the global element count first: the cotangent is scaled by it
        sums, _ = _lib.class_sums(mean, tg, stride, bi, "mse")
        reduce_fn(sums)
        _, gm = _lib.class_sums(mean, tg, stride, bi, "mse", 1.0 / float(sums[2]), True)
    else:
        sums, gm = _lib.class_sums(mean, tg, stride, bi, loss, 1.0 / (b * R) if loss == "mse" else 1.0, True)
        if reduce_fn is not None:
            reduce_fn(sums)
    ce, r2sum, count = (float(v) for v in sums[:3].tolist())
    value = ce if loss == "cross_entropy" else r2sum / count
    g_l, g_n, *g_nu = _hyper_partials(spec, inp, info, gm, None, **({"want_nu": True} if grad_smoothness else {}))
    return (value, *_hyper_gradient(g_l, g_n, info, "classification gradient", reduce_fn, *g_nu))


def loocv_tree_sums(mean: torch.Tensor, var: torch.Tensor, ykinvy: torch.Tensor, train_targets: torch.Tensor,
                    batch_indices: Optional[torch.Tensor], huber_delta: float = 1.5, leaves=(0, 0)) -> torch.Tensor:
    """The LOOCV partial sums from finished outputs (``mgp_loocv_tree_*``): the reduction tree ``mgp_loocv_*`` walks
    inside its fused launch, as three small launches -- equal bits for equal ``leaves`` = ``_lib.last_loocv_geometry()``
    of that call (csrc/mgp_loocv_tree.h).  ``mean`` / ``var`` / ``ykinvy`` ``(b,)`` as returned by
    :func:`posterior_mean_var` with ``want_ykinvy``; one response."""
    _lib.require_cuda(mean, var, ykinvy, train_targets, batch_indices)
    dtype = mean.dtype
    b = mean.numel()
    tg = train_targets.reshape(-1).to(dtype).contiguous()
    bi = None if batch_indices is None else batch_indices.to(torch.int64).contiguous()
    out = torch.empty(6, device=mean.device, dtype=torch.float64)
    scratch = torch.empty(int(_lib.load().mgp_loocv_scratch_bytes()), dtype=torch.uint8, device=mean.device)
    rc = _lib.fn("loocv_tree", dtype)(_lib.ptr(mean.contiguous()), _lib.ptr(var.contiguous()), _lib.ptr(ykinvy.contiguous()),
                                      _lib.ptr(tg), tg.element_size(), _lib.ptr(bi), b, float(huber_delta), int(leaves[0]), int(leaves[1]), _lib.ptr(out),
                                      _lib.ptr(scratch), _lib.stream_ptr())
    _lib.check(rc, "mgp_loocv_tree")
    return out


def fast_posterior_mean(
    spec: KernelSpec,
    test_features: torch.Tensor,
    train_features: torch.Tensor,
    test_indices: Optional[torch.Tensor],
    closest_set: torch.Tensor,
    coeffs: torch.Tensor,
    closest_neighbor: torch.Tensor,
    out: Optional[torch.Tensor] = None,
):
    """Prediction from precomputed coefficients, fused (``mgp_fast_posterior_mean_*``).

    ``closest_set (b, k)`` is the self-including neighbourhood of each test point's closest
    training point ``closest_neighbor (b,)`` and ``coeffs (n_train, k[, R])`` the coefficient
    table (reference workflow: examples/fast_posterior_mean.py:373-400; maths
    _src/gp/muygps/numpy.py:70-77).  Returns ``(b,)`` or ``(b, R)``.  Any ``nn_count``: up to 64 slots one test point per
    32 or 64 lanes, beyond that one test point per wave in passes of 64 neighbours (csrc/mgp_fast_mean.hip);
    :class:`FusedUnsupported` only follows a status the library really returns."""
    refuse_length_scale_batch(spec)
    _lib.require_cuda(coeffs, closest_neighbor)
    inp = _normalize(spec, test_features, train_features, test_indices, closest_set, want_noise=False)
    fq, fn, bi, ni, b, k, d, ls, dtype = inp.fq, inp.fn, inp.bi, inp.ni, inp.b, inp.k, inp.d, inp.ls, inp.fn.dtype
    squeeze = coeffs.ndim == 2
    co = (coeffs[:, :, None] if squeeze else coeffs).to(dtype).contiguous()
    if co.shape[1] != k:
        raise ValueError(f"coefficient rows hold {co.shape[1]} entries but the neighbourhoods have {k}")
    R = co.shape[2]
    crow = closest_neighbor.to(torch.int64).contiguous()
    mean = out if out is not None else torch.empty((b, R), device=fn.device, dtype=dtype)
    # the general-smoothness Matern under gen_fast("fused"): its own entry, the smoothness in place of the kernel id
    # (any other mode: the closed-form entry, which refuses the id as it always has)
    gen = spec.kernel == "matern_gen" and _GEN_FAST == "fused"
    entry = "fast_posterior_mean_gen" if gen else "fast_posterior_mean"
    rc = _lib.fn(entry, dtype)(
        _lib.ptr(fq), _lib.ptr(fn), d, _lib.ptr(bi), _lib.ptr(ni), b, k, _lib.ptr(co), _lib.ptr(crow), R,
        _gen_smoothness(spec) if gen else spec.kernel_id(), spec.metric_id(), _lib.ptr(ls), ls.numel(), _lib.ptr(mean),
        _lib.stream_ptr(),
    )
    if rc == _lib.EUNSUPPORTED:
        model = f"{spec.kernel!r} (smoothness {spec.smoothness})" if gen else repr(spec.kernel)
        raise FusedUnsupported(f"mgp_{entry} refused kernel {model} at nn_count = {k}, {R} response column(s)")
    _lib.check(rc, f"mgp_{entry}")
    return mean.reshape(b) if squeeze else mean


def _fused_coefficients(spec: KernelSpec, inp: _Inputs) -> Optional[torch.Tensor]:
    """``(K_b + eps)^-1 Y_b`` (b, k, R) of the neighbourhoods ``inp.ni`` of one table in ONE launch: the wave kernel
    (``mgp_fast_coefficients_*``: one response, k <= 62) where it serves the shape, else ``mgp_fast_coefficients_any_*``
    (the system in LDS, or on a slab of a workspace beyond ``mgp_max_nn_count``).  None, without a call, for what no fused
    coefficient kernel serves -- the general-smoothness Matern (not a kernel id of the wave entry at all) outside
    :func:`gen_fast` ``"fused"`` and systems of more than 1024 rows (``nn_count + 1 + R``) -- and when the library refuses
    (``MGP_EUNSUPPORTED``): the caller materialises.  Under ``gen_fast("fused")`` the general smoothness takes one
    ``mgp_fast_coefficients_gen_*`` launch."""
    P = _lib.ptr
    fn, b, k, R, dtype = inp.fn, inp.b, inp.k, inp.R, inp.fn.dtype
    gen = spec.kernel == "matern_gen"
    if (gen and _GEN_FAST != "fused") or k + 1 + R > 1024:
        return None
    out = torch.empty((b, k, R), device=fn.device, dtype=dtype)
    info = torch.zeros(1, device=fn.device, dtype=torch.int32)
    if gen:
        # gen_fast("fused"): ONE mgp_fast_coefficients_gen_* launch (the LDS workgroup kernel up to mgp_max_nn_count_gen,
        # no workspace; the slab kernel beyond); None when the library refuses (nu > 30)
        nu = _gen_smoothness(spec)
        ws = _lib.workspace("mgp_fast_coefficients_gen_workspace_bytes", dtype, k, R, b, device=fn.device)
        rc = _lib.fn("fast_coefficients_gen", dtype)(
            P(fn), inp.d, P(inp.ni), b, k, P(inp.tg), R, inp.mode, inp.eps, P(inp.nz), nu, spec.metric_id(), P(inp.ls),
            inp.ls.numel(), P(out), P(info), P(ws), 0 if ws is None else ws.numel(), _lib.stream_ptr(),
        )
        if rc == _lib.EUNSUPPORTED:
            return None
        _lib.check(rc, "mgp_fast_coefficients_gen")
        _lib.raise_if_not_spd(info, "fast_coefficients")
        return out
    model = (inp.mode, inp.eps, P(inp.nz), spec.kernel_id(), spec.metric_id(), P(inp.ls), inp.ls.numel())

    def wave():  # mgp_fast_coefficients_* (fused gather .. LDL^T .. back-substitution on the wave kernel)
        return _lib.fn("fast_coefficients", dtype)(
            P(fn), inp.d, P(inp.ni), b, k, P(inp.tg), *model, P(out), P(info), _lib.stream_ptr(),
        )

    def workgroup():  # (a workspace only beyond LDS: None where the system fits)
        ws = _lib.workspace("mgp_fast_coefficients_workspace_bytes", dtype, k, R, b, device=fn.device)
        return _lib.fn("fast_coefficients_any", dtype)(
            P(fn), inp.d, P(inp.ni), b, k, P(inp.tg), R, *model, P(out), P(info), P(ws), 0 if ws is None else ws.numel(),
            _lib.stream_ptr(),
        )

    rungs = (wave, workgroup) if R == 1 and k <= 62 else (workgroup,)
    rc, at = _lib.run_ladder(rungs)
    if rc == _lib.EUNSUPPORTED:
        return None
    _lib.check(rc, "mgp_fast_coefficients" if rungs[at] is wave else "mgp_fast_coefficients_any")
    _lib.raise_if_not_spd(info, "fast_coefficients")
    return out


def fast_coefficients(spec: KernelSpec, train_features: torch.Tensor, train_targets: torch.Tensor,
                      train_nn_indices: torch.Tensor, chunk: int = 262144, fused: bool = True) -> torch.Tensor:
    """Coefficient table ``C_i = (K_i + eps)^-1 y_i`` over the self-including neighbourhoods
    ``[i, nn[i][:-1]]`` (_fast_nn_update + _muygps_fast_posterior_mean_precompute,
    _src/gp/tensors/numpy.py:97-108, _src/gp/muygps/numpy.py:88-95), computed once per model: one
    fused launch for any ``nn_count`` and response count with ``nn_count + 1 + R <= 1024`` (``mgp_fast_coefficients_*``
    for one response and k <= 62, ``mgp_fast_coefficients_any_*`` otherwise) or, with ``fused=False`` / for what no
    fused kernel serves (the general-smoothness Matern, through ``mgp_matern_gen_*`` -- unless :func:`gen_fast` ``"fused"``
    is in force: then ``mgp_fast_coefficients_gen_*``, one launch; more than 1024 rows), row chunks through the
    per-function kernels.  Returns ``(n, k)`` or ``(n, k, R)`` together with the updated index table
    ``(n, k)``."""
    from muygpys_amd._src.gp.kernels import hip as K
    from muygpys_amd._src.gp.muygps import hip as M
    from muygpys_amd._src.gp.noise import hip as N
    from muygpys_amd._src.gp.tensors import hip as T

    refuse_length_scale_batch(spec)
    _lib.require_cuda(train_features, train_targets, train_nn_indices)
    nn_fast = T._fast_nn_update(train_nn_indices.to(torch.int64))
    n, k = nn_fast.shape
    d = 1 if train_features.ndim == 1 else train_features.shape[1]
    squeeze = train_targets.ndim == 1
    R = 1 if squeeze else train_targets.shape[1]
    if fused:
        inp = _normalize(spec, train_features, train_features, None, nn_fast, train_targets.to(train_features.dtype))
        out = _fused_coefficients(spec, inp)
        if out is not None:
            return (out.reshape(n, k) if squeeze else out), nn_fast
    out = torch.empty((n, k, R), device=train_features.device, dtype=train_features.dtype)
    aniso = not isinstance(spec.length_scale, (int, float)) and len(spec.length_scale) > 1
    gen = spec.kernel == "matern_gen"  # (mgp_kernel_apply_* knows the closed forms only)
    for s in range(0, n, chunk):
        idx = nn_fast[s:s + chunk].contiguous()
        if aniso:
            ls = _length_scale_tensor(spec.length_scale, d, train_features)
            dist = T._reduce(T._pairwise_tensor(train_features, idx), spec.metric_id(), ls)
            Kin = K._matern_gen_fn(dist, spec.smoothness) if gen else K._apply(dist, spec.kernel, 1.0)
        else:
            ell = float(spec.length_scale if isinstance(spec.length_scale, (int, float)) else spec.length_scale[0])
            scale = 1.0 / ell if spec.metric == "l2" else 1.0 / ell**2
            dist = T._pairwise_distances(train_features, idx, spec.metric)
            Kin = K._matern_gen_fn(dist * scale, spec.smoothness) if gen else K._apply(dist, spec.kernel, scale)
        if isinstance(spec.noise, torch.Tensor) and spec.noise.ndim >= 1:
            Kin = N._heteroscedastic_perturb(Kin, spec.noise[idx] if spec.noise.ndim == 1 else spec.noise[s:s + chunk])
        else:
            Kin = N._homoscedastic_perturb(Kin, float(spec.noise))
        Y = train_targets[idx].reshape(idx.shape[0], k, R)
        out[s:s + chunk] = M._solve(Kin, None, Y, want=("coeffs",))[3]
    return (out.reshape(n, k) if squeeze else out), nn_fast
