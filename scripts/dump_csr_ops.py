#!/usr/bin/env python
"""Dump the forward outputs and gradients of the CSR gather ops that the
flagship benchmark does not run, as .npy files, for a byte-for-byte
comparison of two builds of the package (the kernels are bit-reproducible
and order-independent, so any difference between builds is a bug):

  scatter_gather_weighted          out, dx, dw
  scatter_gather_reduce max / min  out, arg, dx
  graph_attention (H = 4)          out, dq, dkv

on the ladder CSR of tests/test_csr_frame_gpu.py, at bf16 D = 64 and fp32
D = 20, from seeded inputs.

  python scripts/dump_csr_ops.py OUTDIR_A
  python scripts/dump_csr_ops.py OUTDIR_B --package-root OTHER_BUILD
  cmp OUTDIR_A/<name>.npy OUTDIR_B/<name>.npy

--package-root names the directory that holds the roc_amd package to dump
(default: this checkout), so one copy of this script and of the test
module's CSR builder serves both builds.
"""
import argparse
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_ap = argparse.ArgumentParser()
_ap.add_argument("outdir")
_ap.add_argument("--package-root", default=ROOT)
ARGS = _ap.parse_args()
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.abspath(ARGS.package_root))

from roc_amd.ops import functional as F  # noqa: E402
from test_csr_frame_gpu import N_SRC, ladder_csr  # noqa: E402

DEV = "cuda:0"
HEADS = 4


def shard():
    rowptr, colidx, t_rowptr, t_colidx, t_eperm = (
        t.to(DEV) for t in ladder_csr())
    n = rowptr.numel() - 1
    gen = torch.Generator().manual_seed(3)
    return types.SimpleNamespace(
        rowptr=rowptr, colidx=colidx, t_rowptr=t_rowptr, t_colidx=t_colidx,
        n_local=n, n_ext=N_SRC,
        row_order=torch.randperm(n, generator=gen).int().to(DEV),
        t_row_order=torch.randperm(N_SRC, generator=gen).int().to(DEV),
        t_edge_perm=lambda: t_eperm.long(), t_edge_perm32=lambda: t_eperm)


def save(outdir, name, t):
    t = t.detach().cpu().contiguous()
    if t.dtype == torch.bfloat16:
        t = t.view(torch.int16)
    np.save(os.path.join(outdir, name + ".npy"), t.numpy())


def main():
    outdir = ARGS.outdir
    os.makedirs(outdir, exist_ok=True)
    print("roc_amd from", os.path.dirname(os.path.abspath(F.__file__)))
    assert F.has_ext() and torch.cuda.is_available()
    sh = shard()
    n, E = sh.n_local, sh.colidx.numel()
    for dtype, D in ((torch.bfloat16, 64), (torch.float32, 20)):
        tag = f"{'bf16' if dtype == torch.bfloat16 else 'fp32'}_D{D}"
        gen = torch.Generator().manual_seed(D)

        def rand(*shape):
            return torch.randn(*shape, generator=gen)

        x = rand(N_SRC, D).to(dtype).to(DEV).requires_grad_(True)
        w = torch.rand(E, generator=gen).to(DEV).requires_grad_(True)
        out = F.scatter_gather_weighted(x, w, sh)
        out.backward(rand(n, D).to(dtype).to(DEV))
        for name, t in (("out", out), ("dx", x.grad), ("dw", w.grad)):
            save(outdir, f"weighted_{tag}_{name}", t)

        for reduce in ("max", "min"):
            x = rand(N_SRC, D).to(dtype).to(DEV).requires_grad_(True)
            out, arg = F.scatter_gather_reduce(x, sh, reduce, return_arg=True)
            out.backward(rand(n, D).to(dtype).to(DEV))
            for name, t in (("out", out), ("arg", arg), ("dx", x.grad)):
                save(outdir, f"{reduce}_{tag}_{name}", t)

        q = rand(n, D).to(dtype).to(DEV).requires_grad_(True)
        kv = rand(N_SRC, 2 * D).to(dtype).to(DEV).requires_grad_(True)
        out = F.graph_attention(q, kv, sh, HEADS)
        out.backward(rand(n, D).to(dtype).to(DEV))
        for name, t in (("out", out), ("dq", q.grad), ("dkv", kv.grad)):
            save(outdir, f"attention_{tag}_{name}", t)
    torch.cuda.synchronize()
    print(f"wrote {len(os.listdir(outdir))} files to {outdir}")


if __name__ == "__main__":
    main()
