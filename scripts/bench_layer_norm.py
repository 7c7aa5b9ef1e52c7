#!/usr/bin/env python3
"""LayerNorm+ReLU microbench: the layer_norm kernels against the torch
composition they replace (torch.nn.functional.layer_norm(...).relu() and
its autograd backward) and against the bytes-moved floor.
Device events, warm-up first, contenders alternate inside every round.
Run on a GPU box:

  python scripts/bench_layer_norm.py [--nodes N --dims D ... --epoch]

Floor: the forward reads x and writes y (2*N*D*elt bytes), the backward
reads dy and x and writes dx (3*N*D*elt); the floor time is those bytes
at --peak-tbs (the measured float4-copy rate of the part, not its spec).
One [N, D] bf16 matrix at the Reddit shape is smaller than the 256 MB
last-level cache, so every call works on the next of a ring of buffer sets
that together exceed --ring-mb: the kernels then stream from HBM, as they
do inside an epoch. A timed window is --inner back-to-back calls.

--epoch adds the epoch time of a 4-layer GCN (hidden 256) on the Reddit
shape with and without --norm layer (timed as scripts/bench_configs.py
does).
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

DEV = "cuda:0"


def run_rounds(contenders, rounds, inner):
    """{name: fn(i)} -> {name: (median ms, best ms)} per call."""
    ev = {k: (torch.cuda.Event(enable_timing=True),
              torch.cuda.Event(enable_timing=True)) for k in contenders}
    times = {k: [] for k in contenders}
    step = 0
    for fn in contenders.values():  # warm
        for i in range(3):
            fn(i)
    torch.cuda.synchronize()
    for _ in range(rounds):
        for k, fn in contenders.items():
            s, e = ev[k]
            s.record()
            for i in range(inner):
                fn(step + i)
            e.record()
            torch.cuda.synchronize()
            times[k].append(s.elapsed_time(e) / inner)
        step += inner
    out = {}
    for k, t in times.items():
        t.sort()
        out[k] = (t[len(t) // 2], t[0])
    return out


def bench_shape(N, D, dtype, rounds, inner, ring_mb, peak_tbs):
    from roc_amd import _C
    elt = torch.empty(0, dtype=dtype).element_size()
    mat = N * D * elt
    # x, dy, y/dx per set (the torch side keeps its own outputs)
    nsets = max(2, int(ring_mb * 1e6 // (3 * mat)) + 1)
    torch.manual_seed(0)
    xs = [torch.randn(N, D, device=DEV).to(dtype) for _ in range(nsets)]
    dys = [torch.randn(N, D, device=DEV).to(dtype) for _ in range(nsets)]
    outs = [torch.empty(N, D, dtype=dtype, device=DEV) for _ in range(nsets)]
    gamma = (torch.randn(D, device=DEV) + 1.0)
    beta = torch.randn(D, device=DEV) * 0.5
    mean = torch.empty(N, dtype=torch.float32, device=DEV)
    rstd = torch.empty_like(mean)
    dgamma, dbeta = torch.empty_like(gamma), torch.empty_like(beta)
    # torch's kernel wants the affine pair in x's dtype
    gt = gamma.to(dtype).requires_grad_(True)
    bt = beta.to(dtype).requires_grad_(True)
    xg = [x.clone().requires_grad_(True) for x in xs]

    def ours_fwd(i):
        k = i % nsets
        _C.layer_norm_fwd(outs[k], None, None, xs[k], gamma, beta, 1e-5, True)

    def ours_fwd_bwd(i):
        k = i % nsets
        _C.layer_norm_fwd(outs[k], mean, rstd, xs[k], gamma, beta, 1e-5, True)
        _C.layer_norm_bwd(outs[k], dgamma, dbeta, dys[k], xs[k], mean, rstd,
                          gamma, beta, True)

    def torch_fwd(i):
        k = i % nsets
        with torch.no_grad():
            torch.nn.functional.layer_norm(xs[k], (D,), gt, bt, 1e-5).relu()

    def torch_fwd_bwd(i):
        k = i % nsets
        xg[k].grad = gt.grad = bt.grad = None
        torch.nn.functional.layer_norm(xg[k], (D,), gt, bt, 1e-5).relu() \
            .backward(dys[k])

    res = run_rounds({"layer_norm fwd": ours_fwd,
                      "layer_norm fwd+bwd": ours_fwd_bwd,
                      "torch layer_norm.relu fwd": torch_fwd,
                      "torch layer_norm.relu fwd+bwd": torch_fwd_bwd},
                     rounds, inner)
    floor = {"fwd": 2 * mat / (peak_tbs * 1e12) * 1e3,
             "fwd+bwd": 5 * mat / (peak_tbs * 1e12) * 1e3}
    name = "bf16" if dtype == torch.bfloat16 else "fp32"
    print(f"== N={N} D={D} {name} ({mat / 1e6:.0f} MB per matrix, ring of "
          f"{nsets} sets) ==", flush=True)
    row = {"N": N, "D": D, "dtype": name}
    for what in ("fwd", "fwd+bwd"):
        ours = res[f"layer_norm {what}"]
        tch = res[f"torch layer_norm.relu {what}"]
        print(f"  {what:8s} ours median {ours[0]:.4f} ms best {ours[1]:.4f} | "
              f"torch median {tch[0]:.4f} ms best {tch[1]:.4f} | floor "
              f"{floor[what]:.4f} ms | torch/ours {tch[0] / ours[0]:.2f}x | "
              f"ours/floor {ours[0] / floor[what]:.2f}x", flush=True)
        row[what] = {"ours_ms": ours[0], "ours_best_ms": ours[1],
                     "torch_ms": tch[0], "torch_best_ms": tch[1],
                     "floor_ms": floor[what]}
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
    for norm in ("none", "layer"):
        model = build_model("gcn", dims, dropout=0.5, seed=1, norm=norm)
        opt = AdamOptimizer(model.parameters(), lr=0.01, weight_decay=1e-4,
                            no_decay=model.norm_parameters())
        trainers[norm] = Trainer(model, shard, feats, labels, mask, opt,
                                 device=DEV, compute_dtype=torch.bfloat16,
                                 num_classes=c, grad_scale=gs)
        for _ in range(warmup):
            trainers[norm].train_epoch()
    times = {"none": [], "layer": []}
    for _ in range(3):  # alternate the two models
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
    ap.add_argument("--dims", type=int, nargs="+", default=[64, 256, 608])
    ap.add_argument("--dtypes", nargs="+", default=["bf16", "fp32"],
                    choices=["bf16", "fp32"])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--ring-mb", type=float, default=600.0)
    ap.add_argument("--peak-tbs", type=float, default=6.29,
                    help="HBM rate the floor is computed at, TB/s")
    ap.add_argument("--epoch", action="store_true")
    ap.add_argument("--epoch-steps", type=int, default=5)
    ap.add_argument("--epoch-warmup", type=int, default=3)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    for name in args.dtypes:
        dtype = torch.bfloat16 if name == "bf16" else torch.float32
        for D in args.dims:
            bench_shape(args.nodes, D, dtype, args.rounds, args.inner,
                        args.ring_mb, args.peak_tbs)
    if args.epoch:
        bench_epoch(args.epoch_steps, args.epoch_warmup)
    print("done")


if __name__ == "__main__":
    main()
