#!/usr/bin/env python3
"""DropEdge aggregation microbench (profiles/r47): the fused drop kernel
(spmm_drop.hip) at several p against (a) the undropped SpMM, one-pass and on
the shard's shipped plan, and (b) the composition that drops edges without
it: a mask, an [E] fp32 weight tensor and scatter_gather_weighted. Forward
and forward + backward, bf16, dst scale on, one process, the variants of one
width interleaved round by round. Run on a GPU box:

  python scripts/bench_spmm_drop.py [--scale S --rounds R --dims .. --ps ..]

--epochs N adds the 2-layer GCN epoch (hidden 256, the Reddit config) with
and without edge_drop = 0.5, N timed epochs after 3 warm-up ones, twice each,
alternating.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch


def time_interleaved(variants, rounds):
    """{name: (median, best)} in ms; every round runs each variant once"""
    for fn in variants.values():  # warm every shape
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    s = torch.cuda.Event(enable_timing=True)
    e = torch.cuda.Event(enable_timing=True)
    for _ in range(rounds):
        for name, fn in variants.items():
            s.record()
            fn()
            e.record()
            torch.cuda.synchronize()
            times[name].append(s.elapsed_time(e))
    return {k: (sorted(v)[len(v) // 2], min(v)) for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0,
                    help="scale of the synthetic Reddit shape")
    ap.add_argument("--epochs", type=int, default=0)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--dims", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--ps", type=float, nargs="+", default=[0.1, 0.5, 0.8])
    args = ap.parse_args()

    from types import SimpleNamespace
    from roc_amd import (AdamOptimizer, Trainer, build_model, build_shard,
                         synthetic_dataset)
    from roc_amd.ops import functional as F

    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    dev = "cuda:0"
    g, feats, labels, mask, c = synthetic_dataset("reddit", seed=1,
                                                  scale=args.scale)
    nodes = g.num_nodes
    cpu_shard = build_shard(g, 0, 1)
    sh = cpu_shard.to(dev)
    # the same shard without its strip plan: the one-pass kernel
    keys = ("rowptr", "colidx", "t_rowptr", "t_colidx", "n_local", "n_ext",
            "row_order", "t_row_order")
    one = SimpleNamespace(**{k: getattr(sh, k) for k in keys},
                          fwd_strips=None, bwd_strips=None)
    rs = sh.rsqrt_deg_local
    E = sh.colidx.numel()
    t_eperm = sh.t_edge_perm()
    print(f"nodes {nodes} edges {E} plan: strips="
          f"{None if sh.fwd_strips is None else len(sh.fwd_strips)} "
          f"ordered={sh.fwd_strip_order is not None}", flush=True)
    F.set_dropout_seed(1)

    for D in args.dims:
        x = torch.randn(nodes, D).to(torch.bfloat16).to(dev)
        gy = torch.randn(nodes, D).to(torch.bfloat16).to(dev)

        def plain(shard, xin=x):
            return F.scatter_gather(xin, shard, dst_scale=rs)

        def drop(p, xin=x):
            return F.scatter_gather(xin, sh, dst_scale=rs, edge_drop=p,
                                    training=True, edge_call_id=0)

        def composed(p, xin=x):
            keep = torch.empty(E, dtype=torch.uint8, device=dev)
            F._C.drop_edge_mask(keep, sh.rowptr, sh.colidx, p, 1, 0)
            w = keep.float() * (1.0 / (1.0 - p))
            return F._SpMMEdge.apply(
                xin, w, sh.rowptr, sh.colidx, sh.t_rowptr, sh.t_colidx,
                t_eperm, sh.n_local, sh.n_ext, rs, sh.row_order,
                sh.t_row_order)

        def with_bwd(fn):
            def run():
                xl = x.detach().requires_grad_(True)
                torch.autograd.grad(fn(xl), xl, gy)
            return run

        fwd = {"spmm one-pass": lambda: plain(one),
               "spmm shipped plan": lambda: plain(sh)}
        for p in args.ps:
            fwd[f"drop p={p}"] = lambda p=p: drop(p)
            fwd[f"mask+weighted p={p}"] = lambda p=p: composed(p)
        both = {"spmm one-pass": with_bwd(lambda xl: plain(one, xl)),
                "spmm shipped plan": with_bwd(lambda xl: plain(sh, xl))}
        for p in args.ps:
            both[f"drop p={p}"] = with_bwd(lambda xl, p=p: drop(p, xl))
            both[f"mask+weighted p={p}"] = with_bwd(
                lambda xl, p=p: composed(p, xl))
        for what, variants in (("fwd", fwd), ("fwd+bwd", both)):
            print(f"== D={D} {what} ==")
            res = time_interleaved(variants, args.rounds)
            for name, (med, best) in res.items():
                print(f"  {name:24s}: median {med:8.3f} ms  best {best:8.3f}",
                      flush=True)
        # the fused path and the composition draw the same mask
        a, b = drop(0.5).float(), composed(0.5).float()
        print(f"  drop vs mask+weighted, p=0.5: relative L2 difference "
              f"{float((a - b).norm() / b.norm()):.2e}")
    if args.epochs:
        feats = torch.nn.functional.pad(feats, (0, (-feats.shape[1]) % 8))
        dims = [feats.shape[1], 256, c + (-c) % 64]
        trainers = {}
        for p in (0.0, 0.5):
            model = build_model("gcn", dims, dropout=0.5, seed=1, edge_drop=p)
            opt = AdamOptimizer(model.parameters(), lr=0.01,
                                weight_decay=1e-4)
            tr = Trainer(model, cpu_shard, feats, labels, mask, opt,
                         device=dev, compute_dtype=torch.bfloat16,
                         num_classes=c,
                         grad_scale=1.0 / max(int((mask == 1).sum()), 1))
            for _ in range(3):
                tr.train_epoch()
            trainers[p] = tr
        print(f"== GCN epoch, dims {dims} ==")
        for rep in range(2):
            for p, tr in trainers.items():
                ms = tr.timed_epochs(args.epochs) / args.epochs * 1e3
                print(f"  edge_drop={p}: {ms:8.3f} ms/epoch (run {rep})",
                      flush=True)
        for p, tr in trainers.items():
            print(f"  edge_drop={p}: ce_loss {tr.evaluate()['ce_loss']:.4f}")
    print("done")


if __name__ == "__main__":
    main()
