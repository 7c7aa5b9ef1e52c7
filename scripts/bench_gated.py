#!/usr/bin/env python3
"""Edge-gated aggregation microbench: the fused gated_agg kernels, both
forms, against one sum SpMM of width D (one gather of half the row bytes, no
gate), seg_softmax (a per-column weight out of one gather, with an online
rescale) and gatv2_attn (4 heads) on the same CSR and D; the ladder depths
each kernel compiles; and, on a graph small enough for its [E, D]
intermediates, the torch index-op composition (ops.reference.gated_aggregate
on the GPU). Device events, warm-up first, contenders alternate inside every
round; medians and bests. Run on a GPU box:

  python scripts/bench_gated.py [--nodes N --edges E --widths 256 64 ...]
"""
import argparse
import os
import sys
from types import SimpleNamespace

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from bench_gatv2 import load_graph, report
from bench_graph_attention import run_rounds

EPS = 1e-6
HEADS = 4  # of the gatv2 contender


def bench_fused(nodes, g, widths, dtype, rounds):
    from roc_amd import _C
    dev = "cuda:0"
    E = g["E"]
    rowptr, colidx, order = g["rowptr"], g["colidx"], g["order"]
    t_rowptr, t_colidx, t_order = g["t_rowptr"], g["t_colidx"], g["t_order"]
    for D in widths:
        torch.manual_seed(0)
        x, q, dy = (torch.randn(nodes, D).to(dtype).to(dev) for _ in range(3))
        kv = torch.randn(nodes, 2 * D).to(dtype).to(dev)
        att = torch.randn(HEADS, D // HEADS, device=dev)
        t = torch.ones(1, device=dev)
        out, dq, dx = (torch.empty_like(q) for _ in range(3))
        dkv = torch.empty_like(kv)
        stats, sm_stats = (torch.empty(nodes, 2 * D, device=dev)
                           for _ in range(2))
        lse = torch.empty(nodes, HEADS, device=dev)
        delta, datt = torch.empty_like(lse), torch.empty_like(att)
        print(f"== nodes={nodes} edges={E} D={D} {dtype} (one [k | val] row "
              f"gather {E * 2 * D * q.element_size() / 1e9:.2f} GB) ==",
              flush=True)

        def fwd(norm, st=True, depth=0):
            _C.gated_agg_fwd(out, stats if norm and st else None, q, kv,
                             rowptr, colidx, order, norm, EPS, depth)

        def dst(norm, depth=0):
            _C.gated_agg_bwd_dst(dq, dy, stats if norm else None, q, kv,
                                 rowptr, colidx, order, norm, depth)

        def src(norm, depth=0):
            _C.gated_agg_bwd_src(dkv, dy, stats if norm else None, q, kv,
                                 t_rowptr, t_colidx, t_order, norm, depth)

        def fwd_bwd(norm):
            fwd(norm)
            dst(norm)
            src(norm)

        def sm_fwd():
            _C.seg_softmax_fwd(out, sm_stats, x, t, rowptr, colidx, order)

        def sm_fwd_bwd():
            sm_fwd()
            _C.seg_softmax_bwd(dx, None, dy, x, sm_stats, t, t_rowptr,
                               t_colidx, t_order)

        def v2_fwd():
            _C.gatv2_attn_fwd(out, lse, x, q, att, rowptr, colidx, order,
                              HEADS, 0.2)

        def v2_fwd_bwd():
            v2_fwd()
            _C.gatv2_attn_bwd_dst(dq, datt, delta, dy, out, lse, x, q, att,
                                  rowptr, colidx, order, HEADS, 0.2)
            _C.gatv2_attn_bwd_src(dx, x, q, att, dy, lse, delta, t_rowptr,
                                  t_colidx, t_order, HEADS, 0.2)

        # the mean form's backward passes read the stats of a mean forward:
        # one runs before they are timed alone, and every contender that
        # writes stats is a mean forward
        fwd(True)
        report(run_rounds({
            "spmm sum, width D": lambda: _C.spmm(out, x, rowptr, colidx, None,
                                                 None, order),
            "seg_softmax fwd + stats": sm_fwd,
            "gatv2 fwd + lse": v2_fwd,
            "gated fwd, sum form": lambda: fwd(False),
            "gated fwd, mean form + stats": lambda: fwd(True),
            "gated fwd, mean form, no stats": lambda: fwd(True, False),
            "gated bwd_dst, sum form": lambda: dst(False),
            "gated bwd_dst, mean form": lambda: dst(True),
            "gated bwd_src, sum form": lambda: src(False),
            "gated bwd_src, mean form": lambda: src(True),
            "gated fwd + bwd, sum form": lambda: fwd_bwd(False),
            "gated fwd + bwd, mean form": lambda: fwd_bwd(True),
            "seg_softmax fwd + bwd": sm_fwd_bwd,
            "gatv2 fwd + bwd": v2_fwd_bwd,
        }, rounds))
        print("  -- ladder depths, mean form --", flush=True)
        fwd(True)
        report(run_rounds({
            "gated fwd + stats, depth 8": lambda: fwd(True, True, 8),
            "gated fwd + stats, depth 16": lambda: fwd(True, True, 16),
            "gated fwd sum form, depth 8": lambda: fwd(False, True, 8),
            "gated fwd sum form, depth 16": lambda: fwd(False, True, 16),
            "gated bwd_dst, depth 8": lambda: dst(True, 8),
            "gated bwd_dst, depth 16": lambda: dst(True, 16),
            "gated bwd_src, depth 4": lambda: src(True, 4),
            "gated bwd_src, depth 8": lambda: src(True, 8),
            "gated bwd_src sum form, depth 4": lambda: src(False, 4),
            "gated bwd_src sum form, depth 8": lambda: src(False, 8),
        }, rounds))


def bench_torch(nodes, edges, widths, dtype, rounds):
    """Fused against the torch composition where its [E, D] tensors fit."""
    from roc_amd.ops import functional as F
    from roc_amd.ops import reference as ref
    dev = "cuda:0"
    g = load_graph(nodes, edges, dev)
    sh = SimpleNamespace(rowptr=g["rowptr"], colidx=g["colidx"],
                         t_rowptr=g["t_rowptr"], t_colidx=g["t_colidx"],
                         n_local=nodes, n_ext=nodes, row_order=g["order"],
                         t_row_order=g["t_order"])
    for D in widths:
        torch.manual_seed(0)
        q = torch.randn(nodes, D).to(dtype).to(dev).requires_grad_(True)
        kv = torch.randn(nodes, 2 * D).to(dtype).to(dev).requires_grad_(True)
        dy = torch.randn(nodes, D).to(dtype).to(dev)
        print(f"== torch composition: nodes={nodes} edges={g['E']} D={D} "
              f"{dtype} (one fp32 [E, D] {g['E'] * D * 4 / 1e9:.2f} GB) ==",
              flush=True)

        def fused(backward):
            o = F.gated_aggregate(q, kv, sh, True, EPS)
            if backward:
                o.backward(dy)

        def composed(backward):
            o = ref.gated_aggregate(q, kv, sh.rowptr, sh.colidx, nodes, True,
                                    EPS)
            if backward:
                o.backward(dy)

        a = F.gated_aggregate(q, kv, sh, True, EPS).float()
        b = ref.gated_aggregate(q, kv, sh.rowptr, sh.colidx, nodes, True,
                                EPS).float()
        print(f"  fused vs composition out: max abs diff "
              f"{float((a - b).abs().max()):.3e} (peak "
              f"{float(b.abs().max()):.3e})", flush=True)
        report(run_rounds({
            "gated fused fwd": lambda: fused(False),
            "torch composition fwd": lambda: composed(False),
            "gated fused fwd + bwd": lambda: fused(True),
            "torch composition fwd + bwd": lambda: composed(True),
        }, rounds))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=232965)
    ap.add_argument("--edges", type=int, default=114848857)
    ap.add_argument("--torch-edges", type=int, default=4000000,
                    help="edges of the graph of the torch comparison "
                         "(0 skips it)")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--widths", type=int, nargs="+", default=[256, 64])
    ap.add_argument("--dtype", choices=["bf16", "fp32"], default="bf16")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float32
    bench_fused(args.nodes, load_graph(args.nodes, args.edges, "cuda:0"),
                args.widths, dtype, args.rounds)
    if args.torch_edges:
        bench_torch(args.nodes, args.torch_edges, args.widths, dtype,
                    args.rounds)
    print("done")


if __name__ == "__main__":
    main()
