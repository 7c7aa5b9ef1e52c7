#!/usr/bin/env python3
"""Max-aggregation microbench: the seg_max kernels against the sum SpMM
(the floor: same gathered bytes, no arg) and against the torch composition
they replace (x[colidx] + scatter_reduce(amax) and its autograd backward).
Device events, warm-up first, contenders alternate inside every round.
Run on a GPU box:

  python scripts/bench_seg_max.py [--nodes N --edges E --dims D ...]

The torch composition materialises [E, D] tensors (a gather in x's dtype
and an int64 index, 10 B per element in bf16, more in its backward), so it
runs only where --torch-budget-gb allows and is reported as "does not fit"
elsewhere. --small-nodes / --small-edges name a second, smaller shape at
which all contenders run.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch


def run_rounds(contenders, rounds):
    """{name: fn} -> {name: (median ms, best ms)}, alternating per round."""
    ev = {k: (torch.cuda.Event(enable_timing=True),
              torch.cuda.Event(enable_timing=True)) for k in contenders}
    times = {k: [] for k in contenders}
    for fn in contenders.values():  # warm
        fn()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for k, fn in contenders.items():
            s, e = ev[k]
            s.record()
            fn()
            e.record()
            torch.cuda.synchronize()
            times[k].append(s.elapsed_time(e))
    out = {}
    for k, t in times.items():
        t.sort()
        out[k] = (t[len(t) // 2], t[0])
    return out


def bench_shape(nodes, edges, D, dtype, rounds, torch_budget_gb):
    from roc_amd import _C
    from roc_amd.graph import build_transpose, synthetic_graph

    dev = "cuda:0"
    g = synthetic_graph(nodes, edges, seed=1)
    E = int(g.colidx.numel())
    t_rp, t_ci = build_transpose(nodes, g.rowptr, g.colidx)
    deg = (g.rowptr[1:] - g.rowptr[:-1])
    t_deg = (t_rp[1:] - t_rp[:-1])
    rowptr, colidx = g.rowptr.to(dev), g.colidx.to(dev)
    t_rowptr, t_colidx = t_rp.to(dev), t_ci.to(dev)
    eperm = torch.argsort(colidx.long(), stable=True).int()
    order = torch.argsort(-deg, stable=True).int().to(dev)
    t_order = torch.argsort(-t_deg, stable=True).int().to(dev)

    torch.manual_seed(0)
    x = torch.randn(nodes, D).to(dtype).to(dev)
    dy = torch.randn(nodes, D).to(dtype).to(dev)
    out = torch.empty_like(x)
    dx = torch.empty_like(x)
    arg = torch.empty(nodes, D, dtype=torch.int32, device=dev)
    esz = x.element_size()
    print(f"== nodes={nodes} edges={E} D={D} {dtype} "
          f"(gather {E * D * esz / 1e9:.2f} GB, arg {nodes * D * 4 / 1e9:.2f}"
          f" GB) ==", flush=True)

    contenders = {
        "spmm sum fwd (floor)":
            lambda: _C.spmm(out, x, rowptr, colidx, None, None, order),
        "seg_max fwd +arg":
            lambda: _C.seg_max_fwd(out, arg, x, rowptr, colidx, order, False),
        "seg_max fwd no arg":
            lambda: _C.seg_max_fwd(out, None, x, rowptr, colidx, order,
                                   False),
        "spmm sum bwd (floor)":
            lambda: _C.spmm(dx, dy, t_rowptr, t_colidx, None, None, t_order),
        "seg_max bwd":
            lambda: _C.seg_max_bwd(dx, dy, arg, t_rowptr, t_colidx, eperm,
                                   t_order),
    }
    # the composition's forward alone holds a gather and an int64 index;
    # its backward adds a mask and gradients of the same shape
    need_gb = E * D * (2 * esz + 8 + 8 + 1) / 1e9
    fits = need_gb <= torch_budget_gb
    if fits:
        ci64 = colidx.long()
        dst = torch.repeat_interleave(
            torch.arange(nodes, device=dev), deg.to(dev))
        xg = x.clone().requires_grad_(True)
        state = {}

        def torch_fwd():
            state["y"] = torch.zeros(nodes, D, dtype=dtype, device=dev) \
                .scatter_reduce(0, dst.unsqueeze(1).expand(E, D), xg[ci64],
                                reduce="amax", include_self=False)

        def torch_fwd_bwd():
            torch_fwd()
            xg.grad = None
            state["y"].backward(dy)

        contenders["torch gather+scatter_reduce fwd"] = torch_fwd
        contenders["torch gather+scatter_reduce fwd+bwd"] = torch_fwd_bwd
    res = run_rounds(contenders, rounds)
    for k, (med, best) in res.items():
        print(f"  {k:38s} median {med:9.3f} ms  best {best:9.3f} ms",
              flush=True)
    if not fits:
        print(f"  torch gather+scatter_reduce              does not fit "
              f"(~{need_gb:.0f} GB of [E, D] intermediates > "
              f"{torch_budget_gb:.0f} GB budget)", flush=True)
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=232965)
    ap.add_argument("--edges", type=int, default=114848857)
    ap.add_argument("--small-nodes", type=int, default=8192)
    ap.add_argument("--small-edges", type=int, default=4000000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--dims", type=int, nargs="+", default=[256])
    ap.add_argument("--dtype", choices=["bf16", "fp32"], default="bf16")
    ap.add_argument("--torch-budget-gb", type=float, default=32.0)
    args = ap.parse_args()
    dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float32
    for D in args.dims:
        if args.small_edges > 0:
            bench_shape(args.small_nodes, args.small_edges, D, dtype,
                        args.rounds, args.torch_budget_gb)
        if args.edges > 0:
            bench_shape(args.nodes, args.edges, D, dtype, args.rounds,
                        args.torch_budget_gb)
    print("done")


if __name__ == "__main__":
    main()
