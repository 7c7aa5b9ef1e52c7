#!/usr/bin/env python3
"""Softmax aggregation microbench (seg_softmax.hip), bf16 at the Reddit
shape: forward alone and forward + backward (x and t both need a gradient)
against

  the sum SpMM        scatter_gather: gathers the same forward bytes
  seg_stats           scatter_gather_stats: the other one-pass aggregator
  the composition     torch index ops over [E, D] tensors with autograd,
                      on a smaller graph (--compose-scale) where they fit

and the gather depths the launchers can run at. Device events, warm-up
first, contenders alternate inside every round; prints the median and the
spread (min .. max) of each. Run on a GPU box:

  python scripts/bench_seg_softmax.py [--dataset reddit --scale 1.0 ...]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from bench_seg_stats import report, run_rounds


def composition(x, t, shard):
    """the softmax aggregation out of torch ops: four [E, D] fp32 tensors"""
    n = shard.n_local
    dst = shard.row_of_edge()
    xs = x.float()[shard.colidx.long()]
    s = t * xs
    m = torch.zeros(n, x.shape[1], device=x.device).scatter_reduce(
        0, dst.unsqueeze(1).expand_as(s), s.detach(), reduce="amax",
        include_self=False)
    p = torch.exp(s - m[dst])
    zeros = torch.zeros(n, x.shape[1], device=x.device)
    out = zeros.index_add(0, dst, p * xs) / zeros.index_add(0, dst, p)
    return out.to(x.dtype)


def bench_dim(shard, D, rounds, warmup, compose):
    from roc_amd import _C
    from roc_amd.ops import functional as F

    dev = shard.rowptr.device
    n, n_src = shard.n_local, shard.n_ext
    E = int(shard.colidx.numel())
    torch.manual_seed(0)
    x = torch.randn(n_src, D).bfloat16().to(dev)
    dy = torch.randn(n, D).bfloat16().to(dev)
    dy4 = torch.randn(n, 4 * D).bfloat16().to(dev)
    xg = x.clone().requires_grad_(True)
    t = torch.ones(1, device=dev, requires_grad=True)
    print(f"== nodes={n} edges={E} D={D} bf16 (one gather of x "
          f"{E * D * 2 / 1e9:.2f} GB) ==", flush=True)

    def fwd_bwd(op, g):
        def run():
            xg.grad = t.grad = None
            op(xg).backward(g)
        return run

    ops = {"softmax": lambda a: F.scatter_gather_softmax(a, shard, t),
           "sum spmm": lambda a: F.scatter_gather(a, shard),
           "seg_stats": lambda a: F.scatter_gather_stats(a, shard)}
    if compose:
        ops = {"softmax": ops["softmax"],
               "composition": lambda a: composition(a, t, shard)}
    with torch.no_grad():
        res = run_rounds({f"{k} fwd": (lambda op=op: op(x))
                          for k, op in ops.items()}, rounds, warmup)
    res.update(run_rounds(
        {f"{k} fwd+bwd": fwd_bwd(op, dy4 if k == "seg_stats" else dy)
         for k, op in ops.items()}, rounds, warmup))
    report(res)
    if compose:
        return
    out = torch.empty(n, D, dtype=x.dtype, device=dev)
    stats = torch.empty(n, 2 * D, dtype=torch.float32, device=dev)
    dx, dt, td = torch.empty_like(x), torch.empty(1, device=dev), t.detach()
    _C.seg_softmax_fwd(out, stats, x, td, shard.rowptr, shard.colidx,
                       shard.row_order)
    depth = {}
    for d in (8, 16):
        depth[f"seg_softmax_fwd depth {d}"] = (
            lambda d=d: _C.seg_softmax_fwd(out, stats, x, td, shard.rowptr,
                                           shard.colidx, shard.row_order, d))
        depth[f"seg_softmax_fwd no stats depth {d}"] = (
            lambda d=d: _C.seg_softmax_fwd(out, None, x, td, shard.rowptr,
                                           shard.colidx, shard.row_order, d))
    for d in (4, 8):
        depth[f"seg_softmax_bwd depth {d}"] = (
            lambda d=d: _C.seg_softmax_bwd(dx, dt, dy, x, stats, td,
                                           shard.t_rowptr, shard.t_colidx,
                                           shard.t_row_order, d))
        depth[f"seg_softmax_bwd no dt depth {d}"] = (
            lambda d=d: _C.seg_softmax_bwd(dx, None, dy, x, stats, td,
                                           shard.t_rowptr, shard.t_colidx,
                                           shard.t_row_order, d))
    report(run_rounds(depth, rounds, warmup))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dataset", default="reddit")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--compose-scale", type=float, default=0.1,
                    help="graph scale of the run against the torch [E, D] "
                         "composition (0 skips it)")
    ap.add_argument("--dims", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    assert args.rounds >= 20, "at least 20 timed repetitions"
    from roc_amd import build_shard, synthetic_dataset

    for scale, compose in ((args.scale, False), (args.compose_scale, True)):
        if scale <= 0:
            continue
        g = synthetic_dataset(args.dataset, seed=1, scale=scale)[0]
        shard = build_shard(g, 0, 1).to("cuda:0")
        for D in args.dims:
            bench_dim(shard, D, args.rounds, args.warmup, compose)
    print("done")


if __name__ == "__main__":
    main()
