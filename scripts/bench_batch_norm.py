#!/usr/bin/env python3
"""BatchNorm+ReLU microbench: the batch_norm kernels against the torch
composition they replace (torch.nn.functional.batch_norm(...).relu() in
training mode and its autograd backward) and against the bytes-moved floor.
Timed as scripts/bench_layer_norm.py times LayerNorm (its run_rounds: device
events, warm-up first, contenders alternate inside every round, a ring of
buffer sets larger than the last-level cache). Run on a GPU box:

  python scripts/bench_batch_norm.py [--nodes N --dims D ... --depth --epoch]

Floor: the forward reads x twice (statistics, apply) and writes y
(3*N*D*elt bytes); the backward reads dy and x twice (column sums, dx) and
writes dx (5*N*D*elt).

--depth times batch_norm_stats and batch_norm_bwd_reduce at 2, 4 and 8
rows in flight per row-group (the choice recorded in docs/KERNELS.md).
--epoch adds the epoch time of a 4-layer GCN (hidden 256) on the Reddit
shape with norm none, layer and sync_batch.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from bench_layer_norm import run_rounds, DEV


def bench_shape(N, D, dtype, rounds, inner, ring_mb, peak_tbs, depth):
    from roc_amd import _C
    elt = torch.empty(0, dtype=dtype).element_size()
    mat = N * D * elt
    nsets = max(2, int(ring_mb * 1e6 // (3 * mat)) + 1)
    torch.manual_seed(0)
    xs = [torch.randn(N, D, device=DEV).to(dtype) for _ in range(nsets)]
    dys = [torch.randn(N, D, device=DEV).to(dtype) for _ in range(nsets)]
    outs = [torch.empty(N, D, dtype=dtype, device=DEV) for _ in range(nsets)]
    gamma = torch.randn(D, device=DEV) + 1.0
    beta = torch.randn(D, device=DEV) * 0.5
    mean, m2, rstd, dgamma, dbeta = (torch.empty(D, device=DEV)
                                     for _ in range(5))
    rm, rv = torch.zeros(D, device=DEV), torch.ones(D, device=DEV)
    gt = gamma.to(dtype).requires_grad_(True)
    bt = beta.to(dtype).requires_grad_(True)
    xg = [x.clone().requires_grad_(True) for x in xs]

    def ours_fwd(i):
        k = i % nsets
        _C.batch_norm_stats(mean, m2, xs[k])
        _C.batch_norm_finalize(rstd, mean, m2, rm, rv, N, 0.1, 1e-5)
        _C.batch_norm_apply(outs[k], xs[k], mean, rstd, gamma, beta, True)

    def ours_fwd_bwd(i):
        k = i % nsets
        ours_fwd(i)
        _C.batch_norm_bwd_reduce(dgamma, dbeta, dys[k], xs[k], mean, rstd,
                                 gamma, beta, True)
        _C.batch_norm_bwd_dx(outs[k], dys[k], xs[k], mean, rstd, gamma, beta,
                             dbeta, dgamma, N, True)

    def torch_fwd(i):
        k = i % nsets
        with torch.no_grad():
            torch.nn.functional.batch_norm(xs[k], rm, rv, gt, bt, True, 0.1,
                                           1e-5).relu()

    def torch_fwd_bwd(i):
        k = i % nsets
        xg[k].grad = gt.grad = bt.grad = None
        torch.nn.functional.batch_norm(xg[k], rm, rv, gt, bt, True, 0.1,
                                       1e-5).relu().backward(dys[k])

    contenders = {"batch_norm fwd": ours_fwd,
                  "batch_norm fwd+bwd": ours_fwd_bwd,
                  "torch batch_norm.relu fwd": torch_fwd,
                  "torch batch_norm.relu fwd+bwd": torch_fwd_bwd}
    if depth:
        _C.batch_norm_stats(mean, m2, xs[0])
        _C.batch_norm_finalize(rstd, mean, m2, None, None, N, 0.1, 1e-5)
        for d in (2, 4, 8):
            contenders[f"stats depth {d}"] = lambda i, d=d: \
                _C.batch_norm_stats(mean, m2, xs[i % nsets], d)
            contenders[f"bwd_reduce depth {d}"] = lambda i, d=d: \
                _C.batch_norm_bwd_reduce(dgamma, dbeta, dys[i % nsets],
                                         xs[i % nsets], mean, rstd, gamma,
                                         beta, True, d)
    res = run_rounds(contenders, rounds, inner)
    floor = {"fwd": 3 * mat / (peak_tbs * 1e12) * 1e3,
             "fwd+bwd": 8 * mat / (peak_tbs * 1e12) * 1e3}
    name = "bf16" if dtype == torch.bfloat16 else "fp32"
    print(f"== N={N} D={D} {name} ({mat / 1e6:.0f} MB per matrix, ring of "
          f"{nsets} sets) ==", flush=True)
    row = {"N": N, "D": D, "dtype": name}
    for what in ("fwd", "fwd+bwd"):
        ours = res[f"batch_norm {what}"]
        tch = res[f"torch batch_norm.relu {what}"]
        print(f"  {what:8s} ours median {ours[0]:.4f} ms best {ours[1]:.4f} | "
              f"torch median {tch[0]:.4f} ms best {tch[1]:.4f} | floor "
              f"{floor[what]:.4f} ms | torch/ours {tch[0] / ours[0]:.2f}x | "
              f"ours/floor {ours[0] / floor[what]:.2f}x", flush=True)
        row[what] = {"ours_ms": ours[0], "ours_best_ms": ours[1],
                     "torch_ms": tch[0], "torch_best_ms": tch[1],
                     "floor_ms": floor[what]}
    for k, v in res.items():
        if "depth" in k:
            print(f"  {k:20s} median {v[0]:.4f} ms best {v[1]:.4f}",
                  flush=True)
            row[k] = v[0]
    print(json.dumps(row), flush=True)
    torch.cuda.synchronize()


def bench_epoch(steps, warmup):
    from roc_amd import (synthetic_dataset, build_shard, build_model,
                         AdamOptimizer, Trainer)
    g, feats, labels, mask, c = synthetic_dataset("reddit", seed=1)
    pad = (-feats.shape[1]) % 8
    if pad:
        feats = torch.nn.functional.pad(feats, (0, pad))
    c_pad = c + ((-c) % 64)
    shard = build_shard(g, 0, 1)
    dims = [feats.shape[1], 256, 256, 256, c_pad]
    gs = 1.0 / max(int((mask == 1).sum()), 1)
    trainers = {}
    for norm in ("none", "layer", "sync_batch"):
        model = build_model("gcn", dims, dropout=0.5, seed=1, norm=norm)
        opt = AdamOptimizer(model.parameters(), lr=0.01, weight_decay=1e-4,
                            no_decay=model.norm_parameters())
        trainers[norm] = Trainer(model, shard, feats, labels, mask, opt,
                                 device=DEV, compute_dtype=torch.bfloat16,
                                 num_classes=c, grad_scale=gs)
        for _ in range(warmup):
            trainers[norm].train_epoch()
    times = {norm: [] for norm in trainers}
    for _ in range(3):  # alternate the models
        for norm, tr in trainers.items():
            times[norm].append(tr.timed_epochs(steps) / steps * 1e3)
    out = {"config": "reddit gcn 4 layers hidden 256 bf16", "dims": dims}
    for norm, t in times.items():
        t.sort()
        out[f"ms_per_epoch_{norm}"] = t[1]
        out[f"ms_per_epoch_{norm}_all"] = [round(v, 3) for v in t]
        out[f"ce_loss_{norm}"] = round(trainers[norm].evaluate()["ce_loss"], 4)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=232965)
    ap.add_argument("--dims", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--dtypes", nargs="+", default=["bf16", "fp32"],
                    choices=["bf16", "fp32"])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--ring-mb", type=float, default=600.0)
    ap.add_argument("--peak-tbs", type=float, default=6.29,
                    help="HBM rate the floor is computed at, TB/s")
    ap.add_argument("--depth", action="store_true")
    ap.add_argument("--epoch", action="store_true")
    ap.add_argument("--epoch-steps", type=int, default=5)
    ap.add_argument("--epoch-warmup", type=int, default=3)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    for name in args.dtypes:
        dtype = torch.bfloat16 if name == "bf16" else torch.float32
        for D in args.dims:
            bench_shape(args.nodes, D, dtype, args.rounds, args.inner,
                        args.ring_mb, args.peak_tbs, args.depth)
    if args.epoch:
        bench_epoch(args.epoch_steps, args.epoch_warmup)
    print("done")


if __name__ == "__main__":
    main()
