"""Dot-product graph attention kernels (graph_attn.hip) against the CPU
composition in float64 on the same bf16-representable values: forward,
dq and both halves of dkv on every team width, the cold path, the online
softmax's rescale on spiked scores, bit-exactness, and GraphTransformer."""
import pytest
import torch

from roc_amd import AdamOptimizer, Trainer, build_model, build_shard
from roc_amd.graph import synthetic_dataset, synthetic_graph
from roc_amd.ops import functional as F
from roc_amd.ops import reference as ref

from test_graph_attention_cpu import (ATT_ROWS, att_hand_graph,
                                      att_hand_values, loop_attention)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N = 3000
_CACHE = {}

FP32_SHAPES = [(1, 4), (3, 20), (4, 64), (1, 256)]
BF16_SHAPES = [(1, 8), (4, 16), (2, 40), (4, 64), (1, 264), (1, 512)]
COLD_SHAPES = [(torch.float32, 4, 2), (torch.bfloat16, 4, 2),
               (torch.bfloat16, 2, 12)]
CASES = ([(torch.float32, h, d) for h, d in FP32_SHAPES]
         + [(torch.bfloat16, h, d) for h, d in BF16_SHAPES] + COLD_SHAPES)


def graph():
    """(cpu shard, gpu shard) of the shared test graph."""
    if "g" not in _CACHE:
        sh = build_shard(synthetic_graph(N, 60000, seed=5), 0, 1)
        _CACHE["g"] = (sh, sh.to(DEV))
    return _CACHE["g"]


def values(heads, dh):
    """bf16-representable fp32 (q, kv, dy) for one shape."""
    key = ("v", heads, dh)
    if key not in _CACHE:
        gen = torch.Generator().manual_seed(100 * heads + dh)
        D = heads * dh
        _CACHE[key] = tuple(
            torch.randn(N, w, generator=gen).bfloat16().float().contiguous()
            for w in (D, 2 * D, D))
    return _CACHE[key]


def reference(q, kv, dy, heads):
    """out, dq, dkv of the CPU composition in float64, over the full
    tensors."""
    sh, _ = graph()
    q = q.double().requires_grad_(True)
    kv = kv.double().requires_grad_(True)
    out = ref.graph_attention(q, kv, sh.rowptr, sh.colidx, N, heads,
                              float(q.shape[1] // heads) ** -0.5)
    out.backward(dy.double())
    return out.detach(), q.grad, kv.grad


def expected(heads, dh):
    key = ("e", heads, dh)
    if key not in _CACHE:
        _CACHE[key] = reference(*values(heads, dh), heads)
    return _CACHE[key]


def run_gpu(q, kv, dy, heads, dtype, backward=True):
    _, shg = graph()
    qg = q.to(dtype).to(DEV).requires_grad_(backward)
    kvg = kv.to(dtype).to(DEV).requires_grad_(backward)
    out = F.graph_attention(qg, kvg, shg, heads)
    assert out.dtype == dtype and out.shape == qg.shape
    if not backward:
        return out.cpu().double(), None, None
    out.backward(dy.to(dtype).to(DEV))
    assert qg.grad.dtype == dtype and kvg.grad.dtype == dtype
    return (out.detach().cpu().double(), qg.grad.cpu().double(),
            kvg.grad.cpu().double())


def check(name, got, want, dtype, grad):
    """The project's tolerances (tests/test_ops_gpu.py)."""
    peak = float(want.abs().max())
    if dtype == torch.float32:
        atol, rtol = peak * 1e-5 + 1e-4, 1e-4
    else:
        atol, rtol = peak * 2 ** -7 + (1e-2 if grad else 1e-3), 0.05
    assert torch.isfinite(got).all(), f"{name}: non-finite values"
    err = (got - want).abs()
    used = float((err / (atol + rtol * want.abs())).max())
    print(f"{name}: max err {float(err.max()):.3e}, peak {peak:.3e}, "
          f"{100 * used:.1f}% of the allowance")
    assert used <= 1.0, f"{name}: {100 * used:.1f}% of the allowance"


def test_inputs_cover_every_rung():
    sh, _ = graph()
    deg = sh.rowptr[1:] - sh.rowptr[:-1]
    # every ladder rung (8, 4, 1) and their tails, and single-edge rows
    assert int(deg.min()) == 1 and int(deg.max()) >= 8 + 4 + 1
    assert int(deg.max()) == 284
    assert set(range(1, 30)) <= set(deg.tolist())
    key = sh.row_of_edge() * N + sh.colidx.long()
    assert key.numel() - key.unique().numel() > 0  # duplicate edges
    t_deg = sh.t_rowptr[1:] - sh.t_rowptr[:-1]
    assert 8 + 4 + 1 <= int(t_deg.max()) < 86
    assert sh.n_ext == N and sh.n_local == N


@pytest.mark.parametrize("dtype,heads,dh", CASES)
def test_forward_backward(dtype, heads, dh):
    q, kv, dy = values(heads, dh)
    want_out, want_dq, want_dkv = expected(heads, dh)
    out, dq, dkv = run_gpu(q, kv, dy, heads, dtype)
    D = heads * dh
    check("out", out, want_out, dtype, False)
    check("dq", dq, want_dq, dtype, True)
    check("dK", dkv[:, :D], want_dkv[:, :D], dtype, True)
    check("dV", dkv[:, D:], want_dkv[:, D:], dtype, True)


# ---------------------------------------------------------------------------
# the rescale branch: bounded random data never proves an online softmax
# ---------------------------------------------------------------------------

SPIKE_H, SPIKE_DH = 4, 64


def spiked():
    """One score 50 or more above the rest of its row, at edge position 0,
    at a middle position past the first group and at the last position
    (one row each): the K row of that source becomes 8 * q[row]."""
    if "spike" not in _CACHE:
        sh, _ = graph()
        q, kv, dy = (t.clone() for t in values(SPIKE_H, SPIKE_DH))
        D = SPIKE_H * SPIKE_DH
        deg = (sh.rowptr[1:] - sh.rowptr[:-1]).tolist()
        col = sh.colidx.tolist()
        scale = SPIKE_DH ** -0.5

        def gap(v, pos):
            """per head: the score at `pos` minus the row's next best"""
            e0 = int(sh.rowptr[v])
            nbrs = col[e0:e0 + deg[v]]
            s = scale * (kv[nbrs, :D].view(-1, SPIKE_H, SPIKE_DH).double()
                         * q[v].view(1, SPIKE_H, SPIKE_DH).double()).sum(2)
            return s[pos] - torch.cat([s[:pos], s[pos + 1:]]).max(0).values

        rows, used = [], set()
        for where in ("first", "middle", "last"):
            for v in range(N):
                if deg[v] < 29 or v in [r for r, _ in rows]:
                    continue
                e0 = int(sh.rowptr[v])
                pos = {"first": 0, "middle": 13, "last": deg[v] - 1}[where]
                u = col[e0 + pos]
                if u in used or col[e0:e0 + deg[v]].count(u) != 1 or u == v:
                    continue
                keep = kv[u, :D].clone()
                kv[u, :D] = 8 * q[v]
                if float(gap(v, pos).min()) < 55:   # a short q[v]: next row
                    kv[u, :D] = keep
                    continue
                used.add(u)
                rows.append((v, pos))
                break
        assert len(rows) == 3
        # with all three in place, every spike stands 50 or more above the
        # rest of its row, in every head
        for v, pos in rows:
            assert float(gap(v, pos).min()) >= 50, (v, pos, gap(v, pos))
        _CACHE["spike"] = (q, kv, dy, reference(q, kv, dy, SPIKE_H))
    return _CACHE["spike"]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_rescale_on_spiked_scores(dtype):
    q, kv, dy, (want_out, want_dq, want_dkv) = spiked()
    fp32 = dtype == torch.float32
    # the bf16 backward is left out on purpose: with `out` rounded to bf16
    # inside delta, an exact emulation already uses 99.8% of the allowance
    out, dq, dkv = run_gpu(q, kv, dy, SPIKE_H, dtype, backward=fp32)
    check("out", out, want_out, dtype, False)
    if fp32:
        D = SPIKE_H * SPIKE_DH
        check("dq", dq, want_dq, dtype, True)
        check("dK", dkv[:, :D], want_dkv[:, :D], dtype, True)
        check("dV", dkv[:, D:], want_dkv[:, D:], dtype, True)


def wide():
    """q scaled by 30: scores span roughly +-170."""
    if "wide" not in _CACHE:
        q, kv, dy = values(SPIKE_H, SPIKE_DH)
        q = (30 * q).bfloat16().float()
        ref_ = reference(q, kv, dy, SPIKE_H)
        _CACHE["wide"] = (q, kv, dy, ref_)
    return _CACHE["wide"]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_wide_score_range(dtype):
    q, kv, dy, (want_out, want_dq, want_dkv) = wide()
    fp32 = dtype == torch.float32
    out, dq, dkv = run_gpu(q, kv, dy, SPIKE_H, dtype, backward=fp32)
    check("out", out, want_out, dtype, False)
    if fp32:
        D = SPIKE_H * SPIKE_DH
        check("dq", dq, want_dq, dtype, True)
        check("dK", dkv[:, :D], want_dkv[:, :D], dtype, True)
        check("dV", dkv[:, D:], want_dkv[:, D:], dtype, True)


# ---------------------------------------------------------------------------
# bit-exactness
# ---------------------------------------------------------------------------

def _raw(dtype, heads, dh, order, with_lse=True):
    """fwd, bwd_dst and bwd_src through _C with a given row order."""
    from roc_amd import _C
    _, shg = graph()
    q, kv, dy = (t.to(dtype).to(DEV) for t in values(heads, dh))
    scale = dh ** -0.5
    fo = to = None
    if order == "reversed":
        fo = torch.arange(N - 1, -1, -1, dtype=torch.int32, device=DEV)
        to = fo.clone()
    out = torch.full_like(q, 7.0)
    lse = torch.full((N, heads), 7.0, device=DEV) if with_lse else None
    _C.graph_attn_fwd(out, lse, q, kv, shg.rowptr, shg.colidx, fo, heads,
                      scale)
    if not with_lse:
        return (out,)
    dq = torch.full_like(q, 7.0)
    delta = torch.full_like(lse, 7.0)
    _C.graph_attn_bwd_dst(dq, delta, dy, out, lse, q, kv, shg.rowptr,
                          shg.colidx, fo, heads, scale)
    dkv = torch.full_like(kv, 7.0)
    _C.graph_attn_bwd_src(dkv, q, dy, lse, delta, kv, shg.t_rowptr,
                          shg.t_colidx, to, heads, scale)
    return out, lse, dq, delta, dkv


# teams of 16 and of 64 lanes honour row_order; a team of 8 drops it
@pytest.mark.parametrize("dtype,heads,dh", [(torch.float32, 4, 64),
                                            (torch.bfloat16, 1, 264),
                                            (torch.bfloat16, 4, 64)])
def test_bit_exact_across_calls_and_row_order(dtype, heads, dh):
    a = _raw(dtype, heads, dh, None)
    b = _raw(dtype, heads, dh, None)
    c = _raw(dtype, heads, dh, "reversed")
    for x, y, z in zip(a, b, c):
        assert torch.equal(x, y)
        assert torch.equal(x, z)
    (no_lse,) = _raw(dtype, heads, dh, None, with_lse=False)
    assert torch.equal(a[0], no_lse)


def test_no_grad_variant_same_bits():
    _, shg = graph()
    q, kv, dy = values(4, 16)
    qg, kvg = q.bfloat16().to(DEV), kv.bfloat16().to(DEV)
    plain = F.graph_attention(qg, kvg, shg, 4)          # lse = None
    qg.requires_grad_(True)
    tracked = F.graph_attention(qg, kvg, shg, 4)        # lse stored
    assert torch.equal(plain, tracked.detach())


# ---------------------------------------------------------------------------
# hand CSR: empty rows, a one-edge row, duplicates, an orphan source
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("dtype,heads,dh", [(torch.float32, 2, 4),
                                            (torch.bfloat16, 2, 8),
                                            (torch.bfloat16, 1, 136),
                                            (torch.float32, 2, 3)])
def test_hand_csr(dtype, heads, dh):
    from roc_amd import _C
    g = att_hand_graph()
    q, kv, dy = att_hand_values(heads, dh)
    want_out, want_dq, want_dkv = loop_attention(q, kv, dy, heads)
    for name in ("rowptr", "colidx", "t_rowptr", "t_colidx"):
        setattr(g, name, getattr(g, name).to(DEV))
    qg = q.to(dtype).to(DEV)
    kvg = kv.to(dtype).to(DEV)
    out = torch.full_like(qg, 7.0)          # empty rows must write zeros
    lse = torch.full((g.n_local, heads), 7.0, device=DEV)
    _C.graph_attn_fwd(out, lse, qg, kvg, g.rowptr, g.colidx, None, heads,
                      dh ** -0.5)
    empty = [v for v, r in enumerate(ATT_ROWS) if not r]
    assert torch.equal(out[empty].cpu(),
                       torch.zeros(len(empty), heads * dh, dtype=dtype))
    check("out", out.cpu().double(), want_out, dtype, False)
    qg.requires_grad_(True)
    kvg.requires_grad_(True)
    F.graph_attention(qg, kvg, g, heads).backward(dy.to(dtype).to(DEV))
    check("dq", qg.grad.cpu().double(), want_dq, dtype, True)
    check("dkv", kvg.grad.cpu().double(), want_dkv, dtype, True)
    assert torch.equal(qg.grad[empty].cpu(),
                       torch.zeros(len(empty), heads * dh, dtype=dtype))
    assert torch.equal(kvg.grad[6].cpu(),
                       torch.zeros(2 * heads * dh, dtype=dtype))  # orphan


def test_no_edges_returns_zeros():
    n = 5
    z64 = torch.zeros(n + 1, dtype=torch.int64, device=DEV)
    z32 = torch.zeros(0, dtype=torch.int32, device=DEV)
    q = torch.randn(n, 16, device=DEV, requires_grad=True)
    kv = torch.randn(n, 32, device=DEV, requires_grad=True)
    out = F.graph_attention_csr(q, kv, z64, z32, z64, z32, n, n, 2)
    out.backward(torch.ones_like(out))
    assert not out.any() and not q.grad.any() and not kv.grad.any()


# ---------------------------------------------------------------------------
# model
# ---------------------------------------------------------------------------

def _dataset(scale, seed):
    g, feats, labels, mask, c = synthetic_dataset("cora", scale=scale,
                                                  seed=seed)
    pad = (-feats.shape[1]) % 8
    if pad:
        feats = torch.nn.functional.pad(feats, (0, pad))
    return g, feats, labels, mask, c, build_shard(g, 0, 1)


def test_transformer_fp32_matches_cpu():
    """One forward + backward in fp32: logits and every parameter gradient
    against the CPU model (the last layer's head of c = 7 columns runs the
    cold path, the hidden one the fast path)."""
    g, feats, labels, mask, c, shard = _dataset(0.15, 9)
    res = {}
    for dev in ("cpu", DEV):
        model = build_model("transformer", [feats.shape[1], 64, c],
                            dropout=0.0, seed=1, heads=4)
        opt = AdamOptimizer(model.parameters(), lr=0.01)
        tr = Trainer(model, shard, feats, labels, mask, opt, device=dev,
                     compute_dtype=torch.float32)
        model.train()
        logits = model(tr.x, tr.shard)
        loss, _ = F.softmax_cross_entropy(logits, tr.labels, tr.mask, 1.0)
        loss.backward()
        res[dev] = (logits.detach().cpu().double(),
                    {n: p.grad.detach().cpu().double()
                     for n, p in model.named_parameters()})
    check("logits", res[DEV][0], res["cpu"][0], torch.float32, False)
    assert len(res["cpu"][1]) == 6
    for name, want in res["cpu"][1].items():
        assert float(want.abs().max()) > 0, name
        check(name, res[DEV][1][name], want, torch.float32, True)


def _bf16_trainer(dropout, seed=11, capture=False):
    g, feats, labels, mask, c, shard = _dataset(0.2, 7)
    model = build_model("transformer", [feats.shape[1], 64, c],
                        dropout=dropout, seed=1, heads=4)
    opt = AdamOptimizer(model.parameters(), lr=0.01, weight_decay=1e-4,
                        decay_rate=0.97, decay_steps=100)
    gs = 1.0 / max(int((mask == 1).sum()), 1)
    tr = Trainer(model, shard, feats, labels, mask, opt, device=DEV,
                 compute_dtype=torch.bfloat16, grad_scale=gs, seed=seed)
    if capture:
        tr.enable_graph_capture(warmup_epochs=2)
    return tr


def test_transformer_trains_bf16():
    tr = _bf16_trainer(0.2)
    m0 = tr.evaluate()
    for _ in range(10):
        tr.train_epoch()
    m1 = tr.evaluate()
    assert m1["ce_loss"] == m1["ce_loss"], "NaN loss"
    assert m1["ce_loss"] < m0["ce_loss"], (m0, m1)


def test_transformer_capture_matches_eager(monkeypatch):
    """Every launch is capturable: 8 replayed epochs against the same
    kernels run eagerly on the device-side schedule (the pattern of
    tests/test_graph_capture_gpu.py)."""
    monkeypatch.setenv("ROC_DETERMINISTIC", "1")
    tr_e = _bf16_trainer(0.0, capture=True)
    tr_e._graph_warmup = 10 ** 9  # device-schedule eager forever
    for _ in range(8):
        tr_e.train_epoch()
    assert tr_e._graph is None
    we = tr_e.model.wq[0].detach().cpu()

    tr_g = _bf16_trainer(0.0, capture=True)
    for _ in range(8):
        tr_g.train_epoch()
    captured = tr_g._graph is not None
    wg = tr_g.model.wq[0].detach().cpu()
    F.set_dropout_counter(None)
    assert captured, "graph was never captured"
    assert torch.allclose(we, wg, atol=1e-5), (we - wg).abs().max()
    assert tr_g.optimizer.t == tr_e.optimizer.t == 8
