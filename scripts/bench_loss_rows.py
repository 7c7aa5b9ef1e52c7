#!/usr/bin/env python3
"""A/B with the shipped kernels: the backward logits SpMM (transpose CSR,
Reddit shape) over the full strip plan against plans without the columns
that are not training rows (partition.build_loss_strip_plan), swept over
the live-column window.

dy is zero on the dropped rows, as softmax_cross_entropy leaves it, so
every pruned result must be torch.equal to the full one; the script
asserts that in every cell. Runs alternate, --rounds of --reps each; one
JSON line per (D, config) with the plan's host setup time.

Run on a GPU box:  python scripts/bench_loss_rows.py
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from roc_amd import synthetic_dataset, build_shard
from roc_amd.graph import MASK_TRAIN
from roc_amd.ops import functional as Fn
from roc_amd.parallel.partition import (build_loss_strip_plan,
                                        build_strip_heavy)

DEV = "cuda:0"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dims", default="64")
    ap.add_argument("--widths", default="16384,24576,32768")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--out", default=None, help="also append the lines here")
    args = ap.parse_args()

    g, _, _, mask, _ = synthetic_dataset("reddit", seed=1, scale=args.scale)
    if args.scale != 1.0:  # small graphs get no strip plan by default
        os.environ.setdefault("ROC_SPMM_STRIP_MIN_EDGES", "1")
    sh = build_shard(g, 0, 1)
    assert sh.bwd_strips is not None and sh.bwd_strip_order is None, \
        "the transpose CSR needs its natural strip plan"
    n, hmin = sh.n_local, sh.strip_heavy_min
    keep = mask == MASK_TRAIN
    full = [(a.to(DEV), b.to(DEV)) for a, b in sh.bwd_strips]
    full_heavy = ([h.to(DEV) for h in sh.bwd_strip_heavy]
                  if sh.bwd_strip_heavy is not None else None)
    plans = {"full": (full, full_heavy)}
    info = {"full": {"strips": len(full), "edges": int(sh.t_colidx.numel())}}
    for w in (int(v) for v in args.widths.split(",")):
        t0 = time.perf_counter()
        strips, _ = build_loss_strip_plan(sh.t_rowptr, sh.t_colidx, keep, w)
        heavy = build_strip_heavy(strips, hmin) if hmin > 0 else None
        setup = time.perf_counter() - t0
        info[f"w{w}"] = {"strips": len(strips), "setup_s": round(setup, 2),
                         "edges": int(sum(c.numel() for _, c in strips))}
        plans[f"w{w}"] = (
            [(a.to(DEV), b.to(DEV)) for a, b in strips],
            [h.to(DEV) for h in heavy] if heavy is not None else None)

    keep_d = keep.to(DEV).unsqueeze(1)
    lines = []
    for D in (int(d) for d in args.dims.split(",")):
        dy = torch.randn(n, D, device=DEV).to(torch.bfloat16)
        dy = dy * keep_d.to(torch.bfloat16)

        def run(name):
            strips, heavy = plans[name]
            return Fn._strip_spmm(dy, strips, sh.n_ext, None, heavy, hmin)

        want = run("full")
        for name in plans:
            assert torch.equal(run(name), want), (D, name)
        times = {k: [] for k in plans}
        for _ in range(args.rounds):
            for name in plans:
                run(name)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.reps):
                    run(name)
                torch.cuda.synchronize()
                times[name].append(
                    (time.perf_counter() - t0) / args.reps * 1e3)
        for name, ts in times.items():
            line = json.dumps({"D": D, "config": name, "equal": True,
                               "ms": [round(v, 4) for v in ts],
                               "min": round(min(ts), 4), **info[name]})
            print(line, flush=True)
            lines.append(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
