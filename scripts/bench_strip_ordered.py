#!/usr/bin/env python3
"""A/B: degree-ordered strip plan with one-pass light rows against the
natural plan with heavy-first lists (forward CSR, Reddit shape).

(a)  today's path: K heavy-first passes, the last one storing bf16.
(b)  one plain bf16 SpMM over the rows with total degree < T, plus K
     plain passes over the rest, rows sorted by degree (descending).
     T = 0 is "ordering alone".

--mode shipped  prices (b) with kernels that know nothing of the plan:
                both parts write compact buffers in plan order, so the
                outputs are not comparable with (a); only time counts.
--mode real     runs (b) through the library path (F._strip_spmm with the
                ordered plan: stores go through the row permutation) and
                checks every output against (a) bit for bit.

Runs alternate, --rounds of each; one JSON line per (D, config).

Run on a GPU box:  python scripts/bench_strip_ordered.py --mode real
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from roc_amd import synthetic_dataset, build_shard
from roc_amd.ops import functional as Fn
from roc_amd.parallel.partition import (build_strip_heavy, build_strip_plan,
                                        build_strip_plan_ordered)

_C = Fn._C
DEV = "cuda:0"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["shipped", "real"], default="real")
    ap.add_argument("--dims", default="256,64")
    ap.add_argument("--thresholds", default="0,64,128,240,480,960")
    ap.add_argument("--width", type=int, default=16384)
    ap.add_argument("--heavy-min", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--out", default=None, help="also append the lines here")
    args = ap.parse_args()

    g, *_ = synthetic_dataset("reddit", seed=1, scale=args.scale)
    sh = build_shard(g, 0, 1)
    n = g.num_nodes
    deg = np.diff(sh.rowptr.numpy())
    nat = build_strip_plan(sh.rowptr, sh.colidx, n, args.width)
    heavy = [h.to(DEV) for h in build_strip_heavy(nat, args.heavy_min)]
    nat = [(a.to(DEV), b.to(DEV)) for a, b in nat]
    # every threshold's plan is a cut of one sorted plan: the heavy region
    # is a row prefix of each strip, the light CSR a suffix of the sorted CSR
    perm, _, strips_all, _ = build_strip_plan_ordered(
        sh.rowptr, sh.colidx, n, args.width, 0)
    _, _, _, (prp, pci) = build_strip_plan_ordered(
        sh.rowptr, sh.colidx, n, args.width, int(deg.max()) + 1)
    cuts = [srp.numpy().copy() for srp, _ in strips_all]
    strips_all = [(a.to(DEV), b.to(DEV)) for a, b in strips_all]
    prp_h = prp.numpy()
    prp, pci, perm = prp.to(DEV), pci.to(DEV), perm.to(DEV)
    scale = sh.rsqrt_deg_local.to(DEV)
    scale_plan = scale[perm.long()].contiguous()

    def plan_for(t):
        nh = n if t <= 0 else int((deg >= t).sum())
        strips = [(srp[:nh + 1], sci[:int(c[nh])])
                  for (srp, sci), c in zip(strips_all, cuts)]
        light = ((prp[nh:] - int(prp_h[nh])).contiguous(),
                 pci[int(prp_h[nh]):])
        return nh, strips, light

    lines = []
    for D in (int(d) for d in args.dims.split(",")):
        x = torch.randn(n, D, device=DEV).to(torch.bfloat16)

        def run_a():
            return Fn._strip_spmm(x, nat, n, scale, heavy, args.heavy_min)

        runs = {"a": run_a}
        info = {"a": {}}
        for t in (int(v) for v in args.thresholds.split(",")):
            nh, strips, light = plan_for(t)
            info[f"T{t}"] = {"n_heavy": nh, "light_edges": int(light[1].numel())}
            if args.mode == "real":
                order = [perm[:nh], perm[nh:], light[0], light[1]]

                def run_b(strips=strips, order=order):
                    return Fn._strip_spmm(x, strips, n, scale, order=order)
            else:
                out_l = torch.empty(n - nh, D, dtype=torch.bfloat16, device=DEV)
                out_h = torch.empty(nh, D, dtype=torch.bfloat16, device=DEV)
                out32 = torch.empty(nh, D, dtype=torch.float32, device=DEV)

                def run_b(nh=nh, strips=strips, light=light, out_l=out_l,
                          out_h=out_h, out32=out32):
                    if nh < n:
                        _C.spmm(out_l, x, light[0], light[1],
                                scale_plan[nh:], None, None)
                    if nh:
                        last = len(strips) - 1
                        for i, (srp, sci) in enumerate(strips):
                            if i == last:
                                _C.spmm(out32, x, srp, sci, scale_plan[:nh],
                                        None, None, i > 0, 0, 0, None, 0,
                                        out_h)
                            else:
                                _C.spmm(out32, x, srp, sci, None, None, None,
                                        i > 0)
                    return None
            runs[f"T{t}"] = run_b

        want = run_a()
        for name, fn in runs.items():
            got = fn()
            if args.mode == "real" and name != "a":
                assert torch.equal(got, want), (D, name)
        times = {k: [] for k in runs}
        for _ in range(args.rounds):
            for name, fn in runs.items():
                fn()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.reps):
                    fn()
                torch.cuda.synchronize()
                times[name].append((time.perf_counter() - t0) / args.reps * 1e3)
        for name, ts in times.items():
            line = json.dumps({"mode": args.mode, "D": D, "config": name,
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
