"""DropEdge on the CPU: the reference Philox against the published
known-answer vectors, the mask over the transpose CSR, the autograd op
against a float64 masked sum, and the undropped route."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from roc_amd.graph import build_transpose
from roc_amd.ops import functional as F
from roc_amd.ops import reference as ref

N_LOCAL, N_EXT = 64, 96
DEGREES = [0, 1, 2, 3, 5, 15, 16, 17, 63, 64, 65, 127, 128, 129, 300]
# chosen on the CPU (drop_conditions below holds for it; the GPU test asserts
# it): at p = 0.9 some non-empty row loses every edge, at p = 0.1 some row of
# degree >= 15 keeps every edge
SEED, OFFSET = 5, 3


def drop_graph():
    """64 rows whose degrees cycle through DEGREES (window and ladder edges of
    spmm_drop.hip: 0, below / at / above 16 and 64, several windows), sources
    drawn from 96 halo-extended ids, so duplicates occur."""
    deg = [DEGREES[i % len(DEGREES)] for i in range(N_LOCAL)]
    rowptr = torch.tensor(np.cumsum([0] + deg), dtype=torch.int64)
    gen = torch.Generator().manual_seed(0)
    colidx = torch.randint(0, N_EXT, (int(rowptr[-1]),), generator=gen,
                           dtype=torch.int32)
    t_rowptr, t_colidx = build_transpose(N_EXT, rowptr, colidx)
    return SimpleNamespace(
        rowptr=rowptr, colidx=colidx, t_rowptr=t_rowptr, t_colidx=t_colidx,
        n_local=N_LOCAL, n_ext=N_EXT, row_order=None, t_row_order=None,
        fwd_strips=None, bwd_strips=None)


def masked_sum64(g, x, keep, p, row_scale=None):
    """(out, S, k) in float64 over the forward CSR: out = row_scale / (1 - p)
    * sum of the kept x rows, S the same sum over |x| with |scale|, k the
    kept count of each row."""
    row = torch.repeat_interleave(torch.arange(g.n_local),
                                  g.rowptr[1:] - g.rowptr[:-1])[keep]
    xs = x.double()[g.colidx.long()[keep]]
    scale = torch.full((g.n_local, 1), 1.0 / (1.0 - p), dtype=torch.float64)
    if row_scale is not None:
        scale = scale * row_scale.double().unsqueeze(1)
    zeros = torch.zeros(g.n_local, x.shape[1], dtype=torch.float64)
    out = zeros.index_add(0, row, xs) * scale
    S = zeros.index_add(0, row, xs.abs()) * scale.abs()
    k = torch.zeros(g.n_local, dtype=torch.float64).index_add(
        0, row, torch.ones(row.numel(), dtype=torch.float64))
    return out, S, k.unsqueeze(1)


def drop_conditions(g):
    deg = g.rowptr[1:] - g.rowptr[:-1]
    row = torch.repeat_interleave(torch.arange(g.n_local), deg)
    kept = {p: torch.zeros(g.n_local, dtype=torch.int64).index_add(
        0, row, ref.drop_edge_mask(g.rowptr, g.colidx, p, SEED,
                                   OFFSET).long()) for p in (0.1, 0.9)}
    return (bool(((deg > 0) & (kept[0.9] == 0)).any())
            and bool(((deg >= 15) & (kept[0.1] == deg)).any()))


@pytest.mark.parametrize("ctr, key, want", [
    # Random123 known-answer vectors of philox4x32_10
    ((0, 0, 0, 0), (0, 0),
     (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2,
     (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344),
     (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
])
def test_philox_known_answers(ctr, key, want):
    got = ref.philox4x32_10([ctr[0] | ctr[1] << 32], ctr[2],
                            key[0] | key[1] << 32, stream=ctr[3])
    assert tuple(int(v) for v in got[0]) == want


def test_transposed_mask_is_forward_mask_permuted():
    g = drop_graph()
    assert drop_conditions(g)
    perm = torch.argsort(g.colidx.long(), stable=True)  # shard.t_edge_perm
    for p in (0.1, 0.5, 0.9):
        fwd = ref.drop_edge_mask(g.rowptr, g.colidx, p, SEED, OFFSET)
        tr = ref.drop_edge_mask(g.t_rowptr, g.t_colidx, p, SEED, OFFSET,
                                transposed=True)
        assert torch.equal(tr, fwd[perm])
        assert 0 < int(fwd.sum()) < fwd.numel()


@pytest.mark.parametrize("p", [0.1, 0.5, 0.9])
def test_cpu_op_matches_float64_masked_sum(p):
    g = drop_graph()
    gen = torch.Generator().manual_seed(1)
    x = torch.randn(N_EXT, 6, generator=gen, dtype=torch.float64,
                    ).requires_grad_()
    rs = torch.rand(N_LOCAL, generator=gen) + 0.5
    dy = torch.randn(N_LOCAL, 6, generator=gen, dtype=torch.float64)
    F.set_dropout_seed(SEED)
    out = F.scatter_gather(x, g, dst_scale=rs, edge_drop=p, training=True,
                           edge_call_id=OFFSET)
    out.backward(dy)
    keep = ref.drop_edge_mask(g.rowptr, g.colidx, p, SEED, OFFSET)
    xr = x.detach().clone().requires_grad_()
    want, _, _ = masked_sum64(g, xr, keep, p, rs)
    want.backward(dy)
    assert torch.allclose(out, want, rtol=1e-12, atol=1e-12)
    assert torch.allclose(x.grad, xr.grad, rtol=1e-12, atol=1e-12)


def test_eval_and_p0_are_the_undropped_path():
    g = drop_graph()
    x = torch.randn(N_EXT, 8, generator=torch.Generator().manual_seed(2))
    plain = F.scatter_gather(x, g)
    assert torch.equal(
        F.scatter_gather(x, g, edge_drop=0.5, training=False), plain)
    assert torch.equal(
        F.scatter_gather(x, g, edge_drop=0.0, training=True), plain)
