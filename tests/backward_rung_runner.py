"""One rung of tests/backward_cases.py on the GPU, in a process of its own: python -m tests.backward_rung_runner --rung F|W|L
--out FILE.  MGP_BACKWARD_DLT and MGP_BACKWARD_LDS are read once per process, so the caller
(tests/test_gpu_backward_rungs.py) sets the rung's environment and starts this module once per rung.

Every case goes through the raw C entries (mgp_posterior_backward_* / mgp_loocv_backward_*).  grad_ls and grad_noise are
pre-filled with NaN (every element of a good neighbourhood must be written), the three accumulated buffers with 0.25
(accumulated into, not overwritten; the caller subtracts it).  Stored in one .npz, per case index i: the outputs
("i/gls", "i/gnz", "i/gq", "i/gnn", "i/gtg" as far as the case passes them), "i/meta" = [return code, info, workgroups,
LDS bytes, return code of mgp_jit_prepare_backward (F; 0 elsewhere)] and "i/name" (mgp_last_kernel_name after the call),
and "ids", the case ids in the order they ran.  No comparison happens here."""

import argparse
import sys

import numpy as np

FILL = 0.25


def _table(torch, x, t, off):
    """A device table; ``off``: its base one element off the 16-byte grid (a flat allocation of one element more)."""
    x = torch.as_tensor(np.array(x), device="cuda").to(t)  # (a copy: the problem is read-only)
    if not off:
        assert x.data_ptr() % 16 == 0
        return x
    flat = torch.empty(x.numel() + 1, dtype=t, device="cuda")
    flat[1:] = x.reshape(-1)
    view = flat[1:].view(x.shape)
    assert view.data_ptr() % 16 == x.element_size() and view.is_contiguous()
    return view


def run_case(c, store, i):
    import torch

    from muygpys_amd import _lib
    from tests import backward_cases as BC

    P = BC.problem(c["id"])
    t = getattr(torch, c["dtype"])
    k, d, R, b = c["k"], c["d"], c["R"], P.b
    dev = lambda a: None if a is None else torch.as_tensor(np.array(a), device="cuda")  # noqa: E731
    fdev = lambda a: None if a is None else dev(a).to(t)  # noqa: E731
    Xn = _table(torch, P.Xn, t, c["off"])
    Xq = _table(torch, P.Xq, t, c["off"]) if c["own_query"] else Xn
    Y, ni = fdev(P.Y), dev(P.ni)
    bi = dev(P.bi) if c["bi"] else None
    ls = fdev(np.atleast_1d(P.ls))
    rows = BC.bad_noise_rows(c, P) if c["bad"] else P.noise_rows
    mode, nd = {"scalar": (_lib.NOISE_SCALAR, None), "table": (_lib.NOISE_TABLE, fdev(P.table)), "batch": (_lib.NOISE_BATCH, fdev(rows))}[c["noise"]]
    gm, gv, gy = fdev(P.gm), fdev(P.gv), fdev(P.gy)
    gls = torch.full((b, ls.numel()), float("nan"), dtype=t, device="cuda")
    gnz = torch.full((b, k), float("nan"), dtype=t, device="cuda")
    want = c["want"]
    gnn = torch.full(P.Xn.shape, FILL, dtype=t, device="cuda") if want in ("all", "nn") else None
    gq = None
    if want == "all":
        gq = torch.full(P.Xq.shape, FILL, dtype=t, device="cuda") if c["own_query"] else gnn
    gtg = torch.full(P.Y.shape, FILL, dtype=t, device="cuda") if want in ("all", "hyper+tg") else None
    if want == "nn":
        gls = gnz = None
    info = torch.zeros(1, dtype=torch.int32, device="cuda")
    kid, mid = _lib.KERNEL_IDS[c["kernel"]], _lib.METRIC_IDS[c["metric"]]
    prep = 0
    if c["rung"] == "F" and BC.prepared_shape(c) is not None:
        prep = int(_lib.load().mgp_jit_prepare_backward(BC.ES[c["dtype"]], k, d, kid))
    p = _lib.ptr
    if c["loocv"]:
        rc = _lib.fn("loocv_backward", t)(p(Xn), d, p(bi), p(ni), b, k, p(Y), mode, BC.NOISE, p(nd), kid, mid, p(ls), ls.numel(), p(gm), p(gv),
                                          p(gy), p(gls), p(gnz), p(info), _lib.stream_ptr())
    else:
        rc = _lib.fn("posterior_backward", t)(p(Xq), p(Xn), d, p(bi), p(ni), b, k, p(Y), R, mode, BC.NOISE, p(nd), kid, mid, p(ls), ls.numel(),
                                              p(gm), p(gv), p(gq), p(gnn), p(gtg), p(gls), p(gnz), p(info), _lib.stream_ptr())
    torch.cuda.synchronize()
    name = _lib.last_kernel()
    workgroups, lds = _lib.last_launch_geometry()
    store[f"{i}/meta"] = np.array([int(rc), int(info.item()), int(workgroups), int(lds), prep], dtype=np.int64)
    store[f"{i}/name"] = np.array(name)
    for key, buf in (("gls", gls), ("gnz", gnz), ("gq", gq if c["own_query"] else None), ("gnn", gnn), ("gtg", gtg)):
        if buf is not None:
            store[f"{i}/{key}"] = buf.cpu().numpy()


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rung", required=True, choices=("F", "W", "L"))
    ap.add_argument("--out", required=True)
    args = ap.parse_args(argv)
    from tests import backward_cases as BC

    cases = BC.rung_cases(args.rung)
    store = {"ids": np.array([c["id"] for c in cases])}
    for i, c in enumerate(cases):
        run_case(c, store, i)
    np.savez(args.out, **store)
    print(f"{args.rung}: {len(cases)} cases stored in {args.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
