"""Max / min neighbor aggregation kernels (seg_max.hip) against the CPU
reference: exact out, exact arg, exact integer gradients."""
import pytest
import torch

from roc_amd import AdamOptimizer, Trainer, build_model, build_shard
from roc_amd.graph import synthetic_dataset, synthetic_graph
from roc_amd.ops import functional as F
from roc_amd.ops import reference as ref

from test_segmax_cpu import HAND_NSRC, hand_case, loop_reference

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N = 3000
_CACHE = {}


def graph():
    """(cpu shard, gpu shard) of the shared test graph."""
    if "g" not in _CACHE:
        sh = build_shard(synthetic_graph(N, 60000, seed=5), 0, 1)
        _CACHE["g"] = (sh, sh.to(DEV))
    return _CACHE["g"]


def features(D):
    """bf16-representable fp32 [N, D]: the first 40 columns are the same
    draw at every D, so the tie count below holds for all of them."""
    if D not in _CACHE:
        torch.manual_seed(1)
        x = torch.randn(N, 40)
        if D > 40:
            x = torch.cat([x, torch.randn(N, D - 40)], 1)
        _CACHE[D] = x[:, :D].bfloat16().float().contiguous()
    return _CACHE[D]


def expected(D, reduce):
    key = (D, reduce)
    if key not in _CACHE:
        sh, _ = graph()
        _CACHE[key] = ref.seg_max(features(D), sh.rowptr, sh.colidx, N,
                                  reduce)
    return _CACHE[key]


def test_inputs_hold_duplicates_and_ties():
    sh, _ = graph()
    deg = sh.rowptr[1:] - sh.rowptr[:-1]
    assert int(deg.max()) >= 16 + 8 + 4 + 1 and int(deg.min()) >= 1
    key = sh.row_of_edge() * N + sh.colidx.long()
    assert key.numel() - key.unique().numel() > 0  # duplicate edges
    out, _ = expected(40, "max")
    winners = int((features(40)[sh.colidx.long()]
                   == out[sh.row_of_edge()]).sum())
    assert winners - out.numel() > 0  # tied winners


@pytest.mark.parametrize("reduce", ["max", "min"])
@pytest.mark.parametrize("dtype,D", [
    (torch.float32, 4), (torch.float32, 41), (torch.float32, 256),
    (torch.float32, 602), (torch.bfloat16, 8), (torch.bfloat16, 40),
    (torch.bfloat16, 256), (torch.bfloat16, 520)])
def test_forward_exact(dtype, D, reduce):
    _, shg = graph()
    want_out, want_arg = expected(D, reduce)
    x = features(D).to(dtype).to(DEV)
    out, arg = F.scatter_gather_reduce(x, shg, reduce, return_arg=True)
    assert out.dtype == dtype and arg.dtype == torch.int32
    assert torch.equal(arg.cpu(), want_arg)
    assert torch.equal(out.cpu(), want_out.to(dtype))


@pytest.mark.parametrize("reduce", ["max", "min"])
@pytest.mark.parametrize("dtype,D", [(torch.float32, 6), (torch.float32, 36),
                                     (torch.bfloat16, 16),
                                     (torch.bfloat16, 136)])
def test_hand_csr(dtype, D, reduce):
    """Empty, all-negative and -inf rows; row_order given equals None bit
    for bit (36 fp32 / 136 bf16 columns put 16 / 32 lanes on a row)."""
    from roc_amd import _C
    g, x = hand_case(D)
    want_out, want_arg = loop_reference(x, reduce)
    xg = x.to(dtype).to(DEV)
    rp, ci = g.rowptr.to(DEV), g.colidx.to(DEV)
    res = []
    for order in (None, torch.arange(g.n_local - 1, -1, -1, dtype=torch.int32,
                                     device=DEV)):
        out = torch.full((g.n_local, D), 7.0, dtype=dtype, device=DEV)
        arg = torch.full((g.n_local, D), 7, dtype=torch.int32, device=DEV)
        _C.seg_max_fwd(out, arg, xg, rp, ci, order, reduce == "min")
        res.append((out.cpu(), arg.cpu()))
    for out, arg in res:
        assert torch.equal(arg, want_arg)
        assert torch.equal(out, want_out.to(dtype))
    # backward on the same case: source 6 has no edge and gets zeros
    g.rowptr, g.colidx = rp, ci
    g.t_rowptr, g.t_colidx = g.t_rowptr.to(DEV), g.t_colidx.to(DEV)
    xg.requires_grad_(True)
    out = F.scatter_gather_reduce(xg, g, reduce)
    dy = torch.randint(-3, 4, (g.n_local, D)).float()
    out.backward(dy.to(dtype).to(DEV))
    want = ref.seg_max_grad(dy, want_arg, None, g.colidx.cpu(), HAND_NSRC)
    assert torch.equal(xg.grad.cpu(), want.to(dtype))


@pytest.mark.parametrize("reduce", ["max", "min"])
@pytest.mark.parametrize("dtype,D", [(torch.float32, 41),
                                     (torch.bfloat16, 40),
                                     (torch.bfloat16, 256)])
def test_backward_exact(dtype, D, reduce):
    sh, shg = graph()
    assert int((sh.t_rowptr[1:] - sh.t_rowptr[:-1]).max()) * 3 <= 256
    _, want_arg = expected(D, reduce)
    torch.manual_seed(D)
    dy = torch.randint(-3, 4, (N, D)).float()  # every partial sum is exact
    want = ref.seg_max_grad(dy, want_arg, sh.rowptr, sh.colidx, N)
    x = features(D).to(dtype).to(DEV).requires_grad_(True)
    out = F.scatter_gather_reduce(x, shg, reduce)
    out.backward(dy.to(dtype).to(DEV))
    assert x.grad.dtype == dtype
    assert torch.equal(x.grad.cpu(), want.to(dtype))


@pytest.mark.parametrize("dtype,D", [(torch.float32, 41),
                                     (torch.bfloat16, 256)])
def test_no_arg_variant_same_bits(dtype, D):
    _, shg = graph()
    x = features(D).to(dtype).to(DEV)
    assert not x.requires_grad
    out = F.scatter_gather_reduce(x, shg, "max")
    assert torch.equal(out.cpu(), expected(D, "max")[0].to(dtype))


def _sage_max_trainer():
    g, feats, labels, mask, c = synthetic_dataset("cora", scale=0.3, seed=2)
    pad = (-feats.shape[1]) % 8
    if pad:
        feats = torch.nn.functional.pad(feats, (0, pad))
    shard = build_shard(g, 0, 1)
    model = build_model("sage", [feats.shape[1], 64, c], dropout=0.2, seed=1,
                        aggr="max")
    opt = AdamOptimizer(model.parameters(), lr=0.01, weight_decay=1e-4)
    gs = 1.0 / max(int((mask == 1).sum()), 1)
    return Trainer(model, shard, feats, labels, mask, opt, device=DEV,
                   compute_dtype=torch.bfloat16, grad_scale=gs)


def test_sage_max_trains_gpu():
    tr = _sage_max_trainer()
    m0 = tr.evaluate()
    for _ in range(30):
        tr.train_epoch()
    m1 = tr.evaluate()
    assert m1["ce_loss"] == m1["ce_loss"], "NaN loss"
    assert m1["ce_loss"] < m0["ce_loss"], (m0, m1)


def test_sage_max_trains_under_graph_capture():
    """Both launches are capturable: the whole epoch replays as a hipGraph."""
    tr = _sage_max_trainer()
    tr.enable_graph_capture(warmup_epochs=2)
    m0 = tr.evaluate()
    for _ in range(30):
        tr.train_epoch()
    captured = tr._graph is not None
    m1 = tr.evaluate()
    F.set_dropout_counter(None)
    assert captured, "the epoch was never captured"
    assert m1["ce_loss"] == m1["ce_loss"], "NaN loss"
    assert m1["ce_loss"] < m0["ce_loss"], (m0, m1)
