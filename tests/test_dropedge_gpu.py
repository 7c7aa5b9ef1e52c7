"""DropEdge on the GPU: the mask kernel against the reference mask bit for
bit, spmm_drop forward and backward against a float64 masked sum, row-order
independence, and GCN(edge_drop=)."""
import pytest
import torch

from roc_amd import build_model, build_shard, synthetic_dataset
from roc_amd.ops import functional as F
from roc_amd.ops import reference as ref

from test_dropedge_cpu import (N_EXT, N_LOCAL, OFFSET, SEED, drop_conditions,
                               drop_graph, masked_sum64)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PS = [0.1, 0.5, 0.9]
# bf16: TEAM 8 / 8 / 32 / 64 with a second column tile; fp32: TEAM 8 / 8 / 64,
# and D = 6, whose second unit straddles D (the cold scalar path)
WIDTHS = [(torch.bfloat16, D) for D in (8, 64, 256, 520)] + \
         [(torch.float32, D) for D in (4, 20, 132, 6)]


@pytest.fixture(scope="module")
def graph():
    g = drop_graph()
    assert drop_conditions(g)
    dev = {k: v.to(DEV) if torch.is_tensor(v) else v
           for k, v in vars(g).items()}
    return g, type(g)(**dev)


@pytest.mark.parametrize("p", PS)
def test_mask_kernel_is_the_reference_mask(graph, p):
    g, gd = graph
    E = g.colidx.numel()
    for rp, ci, tr in ((gd.rowptr, gd.colidx, False),
                       (gd.t_rowptr, gd.t_colidx, True)):
        want = ref.drop_edge_mask(rp.cpu(), ci.cpu(), p, SEED, OFFSET, tr)
        got = torch.empty(E, dtype=torch.uint8, device=DEV)
        F._C.drop_edge_mask(got, rp, ci, p, SEED, OFFSET, None, tr)
        assert torch.equal(got.cpu().bool(), want)
    # counter = c, offset = o is offset = c * 65536 + o
    counter = torch.tensor([7], dtype=torch.int64, device=DEV)
    a = torch.empty(E, dtype=torch.uint8, device=DEV)
    b = torch.empty(E, dtype=torch.uint8, device=DEV)
    F._C.drop_edge_mask(a, gd.rowptr, gd.colidx, p, SEED, OFFSET, counter)
    F._C.drop_edge_mask(b, gd.rowptr, gd.colidx, p, SEED, 7 * 65536 + OFFSET)
    assert torch.equal(a, b)
    want = ref.drop_edge_mask(g.rowptr, g.colidx, p, SEED, 7 * 65536 + OFFSET)
    assert torch.equal(a.cpu().bool(), want)


def _assert_within(got, want, S, k, bf16):
    """|got - want| <= (k + 2) 2^-24 S (+ 2^-8 |want| for a bf16 store): k - 1
    fp32 adds, the fp32 1/(1-p), its product with the row scale and the final
    multiply, each one rounding of a value bounded by S."""
    tol = (k + 2) * 2.0 ** -24 * S + (2.0 ** -8 * want.abs() if bf16 else 0)
    err = (got.double().cpu() - want).abs()
    assert bool((err <= tol).all()), float((err - tol).max())


@pytest.mark.parametrize("scaled", [False, True], ids=["plain", "rowscale"])
@pytest.mark.parametrize("dtype, D", WIDTHS,
                         ids=[f"{'bf16' if t == torch.bfloat16 else 'f32'}-{D}"
                              for t, D in WIDTHS])
@pytest.mark.parametrize("p", PS)
def test_forward_backward_match_float64(graph, p, dtype, D, scaled):
    """The row scales of the bf16 cases are powers of two: the backward
    applies the scale to dy in one row pass that stores bf16, and the bound
    below is the kernel's (fp32 sum, one rounding at the store), so that pass
    has to be exact. The fp32 cases take arbitrary scales."""
    g, gd = graph
    bf16 = dtype == torch.bfloat16
    gen = torch.Generator().manual_seed(D)
    x = torch.randn(N_EXT, D, generator=gen).to(dtype)
    dy = torch.randn(N_LOCAL, D, generator=gen).to(dtype)
    rs = None
    if scaled and bf16:
        rs = 2.0 ** torch.randint(-2, 2, (N_LOCAL,), generator=gen).float()
    elif scaled:
        rs = torch.rand(N_LOCAL, generator=gen) + 0.5
    xd = x.to(DEV).requires_grad_()
    F.set_dropout_seed(SEED)
    out = F.scatter_gather(xd, gd, dst_scale=None if rs is None else rs.to(DEV),
                           edge_drop=p, training=True, edge_call_id=OFFSET)
    out.backward(dy.to(DEV))
    assert out.dtype == dtype and xd.grad.dtype == dtype

    keep = ref.drop_edge_mask(g.rowptr, g.colidx, p, SEED, OFFSET)
    want, S, k = masked_sum64(g, x, keep, p, rs)
    _assert_within(out.detach(), want, S, k, bf16)
    # the gradient: the same sum over the transpose, dy scaled at its source
    t_keep = ref.drop_edge_mask(g.t_rowptr, g.t_colidx, p, SEED, OFFSET, True)
    tg = type(g)(rowptr=g.t_rowptr, colidx=g.t_colidx, n_local=N_EXT)
    dys = dy.double() if rs is None else dy.double() * rs.double().unsqueeze(1)
    want, S, k = masked_sum64(tg, dys, t_keep, p)
    _assert_within(xd.grad, want, S, k, bf16)


def test_row_order_does_not_change_a_bit(graph):
    _, gd = graph
    x = torch.randn(N_EXT, 256, generator=torch.Generator().manual_seed(3),
                    ).bfloat16().to(DEV)
    order = torch.randperm(N_LOCAL, generator=torch.Generator().manual_seed(4),
                           ).int().to(DEV)
    outs = []
    for ro in (None, order):
        out = torch.empty(N_LOCAL, 256, dtype=torch.bfloat16, device=DEV)
        F._C.spmm_drop(out, x, gd.rowptr, gd.colidx, 0.5, SEED, OFFSET, None,
                       None, ro)
        outs.append(out)
    assert torch.equal(outs[0], outs[1])


def test_gcn_edge_drop_trains_differently_and_evaluates_the_same():
    g, feats, _, _, c = synthetic_dataset("cora", scale=0.2, seed=1)
    feats = torch.nn.functional.pad(feats, (0, (-feats.shape[1]) % 8))
    shard = build_shard(g, 0, 1).to(DEV)
    x = feats.to(DEV).bfloat16()
    dims = [feats.shape[1], 64, c]
    F.set_dropout_seed(1)
    out = {}
    for p in (0.0, 0.5):
        model = build_model("gcn", dims, dropout=0.5, seed=1,
                            edge_drop=p).to(DEV)
        with torch.no_grad():
            out[p, "train"] = model.train()(x, shard)
            out[p, "eval"] = model.eval()(x, shard)
    assert torch.equal(out[0.5, "eval"], out[0.0, "eval"])
    assert not torch.equal(out[0.5, "train"], out[0.0, "train"])
    assert bool(torch.isfinite(out[0.5, "train"].float()).all())
