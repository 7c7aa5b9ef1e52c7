#!/usr/bin/env python3
"""PNA aggregation microbench: the one-pass seg_stats kernels against the
composition of existing ops they replace,

  mean = scatter_gather(x, dst_scale=1/deg)
  msq  = scatter_gather(mul(x, x), dst_scale=1/deg)
  max, min = scatter_gather_reduce(x, "max" | "min")
  out  = cat([mean, sqrt(clamp(msq - mean^2, 0) + eps), max, min])

forward alone and forward + backward through autograd, in bf16 at the
Reddit shape. Device events, warm-up first, contenders alternate inside
every round; prints the median and the spread (min .. max) of each. Also
times the gather depths the launchers can run at, and one whole PNA epoch
of configs/reddit_pna_1gpu.yaml. Run on a GPU box:

  python scripts/bench_seg_stats.py [--dataset reddit --scale 1.0 ...]
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch


def run_rounds(contenders, rounds, warmup):
    """{name: fn} -> {name: (median, min, max) ms}, alternating per round."""
    ev = {k: (torch.cuda.Event(enable_timing=True),
              torch.cuda.Event(enable_timing=True)) for k in contenders}
    times = {k: [] for k in contenders}
    for _ in range(warmup):
        for fn in contenders.values():
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
        out[k] = (t[len(t) // 2], t[0], t[-1])
    return out


def report(res):
    for k, (med, lo, hi) in res.items():
        print(f"  {k:34s} median {med:9.3f} ms  spread {hi - lo:7.3f} ms "
              f"({lo:.3f} .. {hi:.3f})", flush=True)


def bench_dim(shard, D, rounds, warmup, eps):
    from roc_amd import _C
    from roc_amd.ops import functional as F

    dev = shard.rowptr.device
    n, n_src = shard.n_local, shard.n_ext
    E = int(shard.colidx.numel())
    torch.manual_seed(0)
    x = torch.randn(n_src, D).bfloat16().to(dev)
    dy = torch.randn(n, 4 * D).bfloat16().to(dev)
    xg = x.clone().requires_grad_(True)
    inv_deg = shard.inv_deg_local
    print(f"== nodes={n} edges={E} D={D} bf16 (one gather of x "
          f"{E * D * 2 / 1e9:.2f} GB) ==", flush=True)

    def composed(t):
        mean = F.scatter_gather(t, shard, dst_scale=inv_deg)
        msq = F.scatter_gather(F.mul(t, t), shard, dst_scale=inv_deg)
        std = torch.sqrt(torch.clamp(msq - mean * mean, min=0) + eps)
        return torch.cat([mean, std,
                          F.scatter_gather_reduce(t, shard, "max"),
                          F.scatter_gather_reduce(t, shard, "min")], 1)

    def fused_fwd_bwd():
        xg.grad = None
        F.scatter_gather_stats(xg, shard, eps).backward(dy)

    def composed_fwd_bwd():
        xg.grad = None
        composed(xg).backward(dy)

    with torch.no_grad():
        res = run_rounds({
            "fused fwd": lambda: F.scatter_gather_stats(x, shard, eps),
            "composition fwd": lambda: composed(x),
        }, rounds, warmup)
    res.update(run_rounds({"fused fwd+bwd": fused_fwd_bwd,
                           "composition fwd+bwd": composed_fwd_bwd},
                          rounds, warmup))
    report(res)
    for what in ("fwd", "fwd+bwd"):
        f, c = res[f"fused {what}"], res[f"composition {what}"]
        print(f"  {what}: fused/composition = {f[0] / c[0]:.3f}, margin "
              f"{c[0] - f[0]:.3f} ms vs composition spread "
              f"{c[2] - c[1]:.3f} ms", flush=True)

    # gather depth of each direction (the kernels alone; the forward with
    # stats + arg saved and without)
    out = torch.empty(n, 4 * D, dtype=x.dtype, device=dev)
    stats = torch.empty(n, 2 * D, dtype=torch.float32, device=dev)
    arg = torch.empty(n, 2 * D, dtype=torch.int32, device=dev)
    dx = torch.empty_like(x)
    eperm = shard.t_edge_perm32()
    _C.seg_stats_fwd(out, stats, arg, x, shard.rowptr, shard.colidx,
                     shard.row_order, eps)
    depth = {}
    for d in (4, 8, 16):
        depth[f"seg_stats_fwd depth {d}"] = (
            lambda d=d: _C.seg_stats_fwd(out, stats, arg, x, shard.rowptr,
                                         shard.colidx, shard.row_order, eps,
                                         d))
        depth[f"seg_stats_fwd alone depth {d}"] = (
            lambda d=d: _C.seg_stats_fwd(out, None, None, x, shard.rowptr,
                                         shard.colidx, shard.row_order, eps,
                                         d))
    for d in (4, 8):  # 16 deep is not compiled: 2.2x slower (profiles/r43)
        depth[f"seg_stats_bwd depth {d}"] = (
            lambda d=d: _C.seg_stats_bwd(dx, dy, x, stats, arg, shard.rowptr,
                                         shard.t_rowptr, shard.t_colidx,
                                         eperm, shard.t_row_order, d))
    report(run_rounds(depth, rounds, warmup))


def bench_epoch(g, feats, labels, mask, num_classes, shard, epochs, hidden):
    from roc_amd import AdamOptimizer, Trainer, build_model, pna_delta

    pad = (-feats.shape[1]) % 8
    if pad:
        feats = torch.nn.functional.pad(feats, (0, pad))
    c_pad = num_classes + ((-num_classes) % 64)
    model = build_model("pna", [feats.shape[1], hidden, c_pad], dropout=0.5,
                        seed=1, delta=pna_delta(g))
    opt = AdamOptimizer(model.parameters(), lr=0.01, weight_decay=1e-4)
    tr = Trainer(model, shard, feats, labels, mask, opt, device="cuda:0",
                 compute_dtype=torch.bfloat16, num_classes=num_classes)
    tr.enable_graph_capture()
    for _ in range(4):
        tr.train_epoch()
    tr.sync()
    times = []
    for _ in range(epochs):
        t0 = time.perf_counter()
        tr.train_epoch()
        tr.sync()
        times.append((time.perf_counter() - t0) * 1e3)
    times.sort()
    print(f"== PNA epoch (2 layers, hidden {hidden}, bf16, captured="
          f"{tr._graph is not None}) ==\n  median {times[len(times) // 2]:.3f}"
          f" ms  spread {times[-1] - times[0]:.3f} ms over {epochs} epochs",
          flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dataset", default="reddit")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--dims", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--epochs", type=int, default=20,
                    help="timed PNA epochs (0 skips the epoch)")
    ap.add_argument("--hidden", type=int, default=256)
    ap.add_argument("--eps", type=float, default=1e-5)
    args = ap.parse_args()
    assert args.rounds >= 20, "at least 20 timed repetitions"
    from roc_amd import build_shard, synthetic_dataset

    g, feats, labels, mask, c = synthetic_dataset(
        args.dataset, seed=1, scale=args.scale, learnable_labels=True)
    shard = build_shard(g, 0, 1)
    shard_dev = shard.to("cuda:0")
    for D in args.dims:
        bench_dim(shard_dev, D, args.rounds, args.warmup, args.eps)
    if args.epochs > 0:
        bench_epoch(g, feats, labels, mask, c, shard, args.epochs,
                    args.hidden)
    print("done")


if __name__ == "__main__":
    main()
