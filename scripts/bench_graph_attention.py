#!/usr/bin/env python3
"""Dot-product graph attention microbench: the fused graph_attn kernels
against the per-head composition of the existing edge kernels (edge_dot ->
edge_softmax -> spmm_edge and their backward, with fp32 [E] tensors in
between) and against two sum SpMMs of width D, the floor: they gather the
same K + V bytes. All contenders read the same random q / kv / dy. Device
events, warm-up first, contenders alternate inside every round.
Run on a GPU box:

  python scripts/bench_graph_attention.py [--nodes N --edges E ...]

--shapes takes HxDH pairs (default 4x64 1x256, the two layers' shapes of
the Reddit config at hidden 256).
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


def bench_graph(nodes, edges, shapes, dtype, rounds):
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
    eperm = torch.argsort(colidx.long(), stable=True)
    order = torch.argsort(-deg, stable=True).int().to(dev)
    t_order = torch.argsort(-t_deg, stable=True).int().to(dev)

    for H, dh in shapes:
        D = H * dh
        scale = dh ** -0.5
        torch.manual_seed(0)
        q = torch.randn(nodes, D).to(dtype).to(dev)
        kv = torch.randn(nodes, 2 * D).to(dtype).to(dev)
        dy = torch.randn(nodes, D).to(dtype).to(dev)
        out = torch.empty_like(q)
        dq = torch.empty_like(q)
        dkv = torch.empty_like(kv)
        lse = torch.empty(nodes, H, dtype=torch.float32, device=dev)
        delta = torch.empty_like(lse)
        esz = q.element_size()
        print(f"== nodes={nodes} edges={E} H={H} dh={dh} {dtype} "
              f"(K+V gather {2 * E * D * esz / 1e9:.2f} GB, one fp32 [E] "
              f"{E * 4 / 1e9:.2f} GB) ==", flush=True)

        def fused_fwd():
            _C.graph_attn_fwd(out, lse, q, kv, rowptr, colidx, order, H,
                              scale)

        def fused_fwd_nolse():
            _C.graph_attn_fwd(out, None, q, kv, rowptr, colidx, order, H,
                              scale)

        def fused_bwd():
            _C.graph_attn_bwd_dst(dq, delta, dy, out, lse, q, kv, rowptr,
                                  colidx, order, H, scale)
            _C.graph_attn_bwd_src(dkv, q, dy, lse, delta, kv, t_rowptr,
                                  t_colidx, t_order, H, scale)

        def fused_fwd_bwd():
            fused_fwd()
            fused_bwd()

        # the composition works on per-head contiguous slices; slicing is
        # part of what it costs (models/gat.py pays the same copies)
        s = torch.empty(E, dtype=torch.float32, device=dev)
        alpha = [torch.empty(E, dtype=torch.float32, device=dev)
                 for _ in range(H)]
        dal = torch.empty(E, dtype=torch.float32, device=dev)
        ds = torch.empty(E, dtype=torch.float32, device=dev)
        oh = torch.empty(nodes, dh, dtype=dtype, device=dev)
        gh = torch.empty(nodes, dh, dtype=dtype, device=dev)

        def heads_of(x, base=0):
            return [x[:, base + k * dh: base + (k + 1) * dh].contiguous()
                    for k in range(H)]

        def comp_fwd():
            qs, ks, vs = heads_of(q), heads_of(kv), heads_of(kv, D)
            for k in range(H):
                _C.edge_dot(s, qs[k], ks[k], rowptr, colidx)
                s.mul_(scale)
                _C.edge_softmax_fwd(alpha[k], s, rowptr)
                _C.spmm_edge(oh, vs[k], rowptr, colidx, alpha[k], None, order,
                             False)
                out[:, k * dh:(k + 1) * dh] = oh

        def comp_bwd():
            qs, ks, vs = heads_of(q), heads_of(kv), heads_of(kv, D)
            gs = heads_of(dy)
            for k in range(H):
                _C.edge_dot(dal, gs[k], vs[k], rowptr, colidx)
                _C.edge_softmax_bwd(ds, dal, alpha[k], rowptr)
                ds.mul_(scale)
                _C.spmm_edge(oh, ks[k], rowptr, colidx, ds, None, order, False)
                dq[:, k * dh:(k + 1) * dh] = oh
                _C.spmm_edge(gh, qs[k], t_rowptr, t_colidx,
                             ds[eperm].contiguous(), None, t_order, False)
                dkv[:, k * dh:(k + 1) * dh] = gh
                _C.spmm_edge(gh, gs[k], t_rowptr, t_colidx,
                             alpha[k][eperm].contiguous(), None, t_order,
                             False)
                dkv[:, D + k * dh: D + (k + 1) * dh] = gh

        def comp_fwd_bwd():
            comp_fwd()
            comp_bwd()

        kmat = kv[:, :D].contiguous()
        vmat = kv[:, D:].contiguous()

        def floor():
            _C.spmm(out, kmat, rowptr, colidx, None, None, order)
            _C.spmm(dq, vmat, rowptr, colidx, None, None, order)

        contenders = {
            "2x spmm sum, width D (floor)": floor,
            "graph_attn fwd + lse": fused_fwd,
            "graph_attn fwd, no lse": fused_fwd_nolse,
            "graph_attn fwd + bwd": fused_fwd_bwd,
            "composition fwd": comp_fwd,
            "composition fwd + bwd": comp_fwd_bwd,
        }
        # the fused and the composed results must agree before any timing
        fused_fwd_bwd()
        ref_out, ref_dq, ref_dkv = out.clone(), dq.clone(), dkv.clone()
        comp_fwd_bwd()
        for name, a, b in (("out", out, ref_out), ("dq", dq, ref_dq),
                           ("dkv", dkv, ref_dkv)):
            err = float((a.float() - b.float()).abs().max())
            print(f"  fused vs composition {name}: max abs diff {err:.3e} "
                  f"(peak {float(b.float().abs().max()):.3e})", flush=True)
        res = run_rounds(contenders, rounds)
        for k, (med, best) in res.items():
            print(f"  {k:32s} median {med:9.3f} ms  best {best:9.3f} ms",
                  flush=True)
        torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=232965)
    ap.add_argument("--edges", type=int, default=114848857)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--shapes", nargs="+", default=["4x64", "1x256"],
                    help="HEADSxHEAD_DIM pairs")
    ap.add_argument("--dtype", choices=["bf16", "fp32"], default="bf16")
    args = ap.parse_args()
    dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float32
    shapes = [tuple(int(v) for v in s.split("x")) for s in args.shapes]
    bench_graph(args.nodes, args.edges, shapes, dtype, args.rounds)
    print("done")


if __name__ == "__main__":
    main()
