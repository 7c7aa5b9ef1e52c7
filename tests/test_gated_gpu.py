"""The edge-gated aggregation kernels (gated_agg.hip) against
ref.gated_aggregate in fp64 on the same bf16-representable values: both
forms on every team width, the cold paths, saturated gates, the hand CSR,
bit-exactness, and GatedGCN on the GPU. The fp64 references of the shared
graph run on the device to keep the tests short."""
from types import SimpleNamespace

import pytest
import torch

from roc_amd import AdamOptimizer, Trainer, build_model, build_shard
from roc_amd.graph import build_transpose, synthetic_dataset
from roc_amd.ops import functional as F
from roc_amd.ops import reference as ref

from test_graph_attention_gpu import DEV, N, check, graph
from test_segsoftmax_gpu import to_dev
from test_segstats_cpu import STATS_NSRC, stats_hand_case

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
FORMS = [False, True]
CASES = [(F32, 4), (F32, 41), (F32, 256), (BF16, 8), (BF16, 40), (BF16, 256),
         (BF16, 520)]
HAND = [(F32, 6), (F32, 36), (BF16, 7), (BF16, 12), (BF16, 136)]
EPS = 1e-6
_CACHE = {}


def values(rows, nsrc, D, seed):
    """bf16-representable fp32 (q, kv, dy), so that one reference serves
    both dtypes"""
    gen = torch.Generator().manual_seed(seed)
    return tuple(torch.randn(n, w, generator=gen).bfloat16().float()
                 for n, w in ((rows, D), (nsrc, 2 * D), (rows, D)))


def expected(g, q, kv, dy, normalize, dev="cpu"):
    """fp64 (out, stats, dq, dkv); stats = [den | out], den = the gate sum
    (the sum form over values of one) + eps, 0 on an empty row"""
    rp, ci = g.rowptr.to(dev), g.colidx.to(dev)
    q = q.to(dev, torch.float64).requires_grad_(True)
    kv = kv.to(dev, torch.float64).requires_grad_(True)
    out = ref.gated_aggregate(q, kv, rp, ci, g.n_local, normalize, EPS)
    out.backward(dy.to(dev, torch.float64))
    with torch.no_grad():
        k = kv[:, :q.shape[1]]
        l = ref.gated_aggregate(q, torch.cat([k, torch.ones_like(k)], 1), rp,
                                ci, g.n_local, False)
        den = (l + EPS) * (rp[1:] > rp[:-1]).unsqueeze(1)
        stats = torch.cat([den, out], 1)
    return tuple(t.detach().cpu() for t in (out, stats, q.grad, kv.grad))


def graph_case(D, normalize):
    key = (D, normalize)
    if key not in _CACHE:
        vals = _CACHE.setdefault(("v", D), values(N, N, D, D))
        _CACHE[key] = vals + (expected(graph()[0], *vals, normalize, DEV),)
    return _CACHE[key]


def run_op(g, q, kv, dy, dtype, normalize):
    """(out, dq, dkv) of the op on the GPU"""
    qg = q.to(dtype).to(DEV).requires_grad_(True)
    kvg = kv.to(dtype).to(DEV).requires_grad_(True)
    out = F.gated_aggregate(qg, kvg, g, normalize, EPS)
    assert out.dtype == dtype and out.shape == qg.shape
    out.backward(dy.to(dtype).to(DEV))
    assert qg.grad.dtype == dtype and kvg.grad.dtype == dtype
    return out.detach().cpu(), qg.grad.cpu(), kvg.grad.cpu()


def check_all(got, want, dtype):
    D = got[0].shape[1]
    out, _, dq, dkv = want
    check("out", got[0].double(), out, dtype, False)
    check("dq", got[1].double(), dq, dtype, True)
    check("dk", got[2][:, :D].double(), dkv[:, :D], dtype, True)
    check("dval", got[2][:, D:].double(), dkv[:, D:], dtype, True)


def launch_fwd(g, q, kv, dtype, normalize, order=None, stats=True):
    """the launcher itself, over poisoned outputs"""
    from roc_amd import _C
    out = torch.full(q.shape, 7.0, dtype=dtype, device=DEV)
    st = torch.full((q.shape[0], 2 * q.shape[1]), 7.0, device=DEV) \
        if stats and normalize else None
    _C.gated_agg_fwd(out, st, q.to(dtype).to(DEV), kv.to(dtype).to(DEV),
                     g.rowptr, g.colidx, order, normalize, EPS)
    return out.cpu(), None if st is None else st.cpu()


@pytest.mark.parametrize("normalize", FORMS)
@pytest.mark.parametrize("dtype,D", CASES)
def test_forward_backward(dtype, D, normalize):
    """520 bf16 columns are three column tiles, the last partly idle; 41
    fp32 columns end in a straddling unit."""
    _, shg = graph()
    q, kv, dy, want = graph_case(D, normalize)
    got = run_op(shg, q, kv, dy, dtype, normalize)
    check_all(got, want, dtype)
    # the saved state, unrounded in both dtypes, and the variant without it
    out, stats = launch_fwd(shg, q, kv, dtype, normalize, shg.row_order)
    assert torch.equal(out, got[0])
    assert torch.equal(launch_fwd(shg, q, kv, dtype, normalize,
                                  shg.row_order, stats=False)[0], out)
    if normalize:
        check("stats", stats.double(), want[1], F32, False)


def saturated_case(kind, normalize):
    """One row of 40 edges over 8 columns: q + k runs from -170 to 170 in
    shuffled order ("span"), or every pre-activation is <= -120 ("low": the
    gate sum is far below eps)."""
    if (kind, normalize) not in _CACHE:
        q, kv, dy = values(1, 40, 8, 7)
        if kind == "span":
            kv[:, :8] += torch.linspace(-170.0, 170.0, 40)[torch.randperm(
                40, generator=torch.Generator().manual_seed(8))].unsqueeze(1)
        else:
            kv[:, :8] = -130.0 - kv[:, :8].abs()
            q = -q.abs()
        kv = kv.bfloat16().float()
        rowptr = torch.tensor([0, 40])
        colidx = torch.arange(40, dtype=torch.int32)
        t_rowptr, t_colidx = build_transpose(40, rowptr, colidx)
        g = SimpleNamespace(rowptr=rowptr, colidx=colidx, t_rowptr=t_rowptr,
                            t_colidx=t_colidx, n_local=1, n_ext=40,
                            row_order=None, t_row_order=None)
        _CACHE[kind, normalize] = (g, q, kv, dy,
                                   expected(g, q, kv, dy, normalize))
    return _CACHE[kind, normalize]


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("normalize", FORMS)
@pytest.mark.parametrize("kind", ["span", "low"])
def test_saturated_gates_stay_finite(kind, normalize, dtype):
    """exp(-z) overflows below z = -88 and the gate is 0 exactly; check()
    asserts finiteness of out, dq and dkv."""
    g, q, kv, dy, want = saturated_case(kind, normalize)
    if kind == "low":
        assert float((q + kv[:, :8]).max()) <= -120.0
    check_all(run_op(to_dev(g), q, kv, dy, dtype, normalize), want, dtype)


@pytest.mark.parametrize("normalize", FORMS)
@pytest.mark.parametrize("dtype,D", HAND)
def test_hand_csr(dtype, D, normalize):
    """Empty rows, duplicate edges, a source without out-edges. 36 fp32 /
    136 bf16 columns put 16 / 32 lanes on a row, so row_order applies; 7
    bf16 columns are rows without 4-B alignment, 12 a full unit and a
    straddling one. Reversing the orders changes no bit."""
    g, _ = stats_hand_case(D)
    q, kv, dy = values(g.n_local, STATS_NSRC, D, 100 + D)
    want = expected(g, q, kv, dy, normalize)
    gg = to_dev(g)
    got = run_op(gg, q, kv, dy, dtype, normalize)
    check_all(got, want, dtype)
    rev = to_dev(g)
    rev.row_order, rev.t_row_order = (
        torch.arange(n - 1, -1, -1, dtype=torch.int32, device=DEV)
        for n in (g.n_local, STATS_NSRC))
    for a, b in zip(got, run_op(rev, q, kv, dy, dtype, normalize)):
        assert torch.equal(a, b)
    out, stats = launch_fwd(gg, q, kv, dtype, normalize)
    rout, rstats = launch_fwd(gg, q, kv, dtype, normalize, rev.row_order)
    assert torch.equal(out, got[0]) and torch.equal(rout, out)
    if normalize:
        check("stats", stats.double(), want[1], F32, False)
        assert torch.equal(rstats, stats) and not stats[0].any()
    assert not out[0].any() and not got[1][0].any()  # the empty row
    assert not got[2][STATS_NSRC - 1].any()  # the source without out-edges


@pytest.mark.parametrize("normalize", FORMS)
def test_runs_and_row_orders_are_bit_identical(normalize):
    _, shg = graph()
    q, kv, dy, _ = graph_case(256, normalize)
    rev = to_dev(shg)
    rev.row_order = rev.t_row_order = torch.arange(
        N - 1, -1, -1, dtype=torch.int32, device=DEV)
    runs = [run_op(g, q, kv, dy, BF16, normalize) for g in (shg, shg, rev)]
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            assert torch.equal(a, b)
    with torch.no_grad():  # the variant without the state stores
        bare = F.gated_aggregate(q.bfloat16().to(DEV), kv.bfloat16().to(DEV),
                                 shg, normalize, EPS)
    assert torch.equal(bare.cpu(), runs[0][0])


def test_no_edges_and_bad_arguments():
    n = 5
    z64 = torch.zeros(n + 1, dtype=torch.int64, device=DEV)
    z32 = torch.zeros(0, dtype=torch.int32, device=DEV)
    q = torch.randn(n, 16, device=DEV, requires_grad=True)
    kv = torch.randn(n, 32, device=DEV, requires_grad=True)
    out = F.gated_aggregate_csr(q, kv, z64, z32, z64, z32, n, n)
    out.backward(torch.ones_like(out))
    assert not out.any() and not q.grad.any() and not kv.grad.any()
    _, shg = graph()
    with pytest.raises(ValueError, match="kv must be"):
        F.gated_aggregate(torch.zeros(N, 8, device=DEV),
                          torch.zeros(N - 1, 16, device=DEV), shg)
    with pytest.raises(ValueError, match="bf16 or fp32"):
        F.gated_aggregate(torch.zeros(N, 8, device=DEV, dtype=torch.half),
                          torch.zeros(N, 16, device=DEV, dtype=torch.half),
                          shg)


@pytest.mark.parametrize("capture", [False, True])
def test_gatedgcn_trains_gpu(capture):
    """Eagerly, and with the whole epoch replayed as a hipGraph: every
    launch is capturable."""
    g, feats, labels, mask, c = synthetic_dataset("reddit", scale=0.01,
                                                  seed=5)
    feats = torch.nn.functional.pad(feats, (0, (-feats.shape[1]) % 8))
    model = build_model("gatedgcn", [feats.shape[1], 64, c + (-c) % 64],
                        dropout=0.3, seed=1, norm="layer")
    opt = AdamOptimizer(model.parameters(), lr=0.01, weight_decay=1e-4,
                        no_decay=model.norm_parameters())
    tr = Trainer(model, build_shard(g, 0, 1), feats, labels, mask, opt,
                 device=DEV, compute_dtype=BF16, num_classes=c,
                 grad_scale=1.0 / max(int((mask == 1).sum()), 1))
    if capture:
        tr.enable_graph_capture(warmup_epochs=2)
    m0 = tr.evaluate()
    for _ in range(6):
        tr.train_epoch()
    captured = capture and tr._graph is not None
    m1 = tr.evaluate()
    F.set_dropout_counter(None)
    assert captured == capture, "the epoch was never captured"
    assert m1["ce_loss"] == m1["ce_loss"], "NaN loss"
    assert m1["ce_loss"] < m0["ce_loss"] * 1.05, (m0, m1)
