"""GATv2 attention kernels (gatv2_attn.hip) against the CPU composition in
float64 on bf16-representable values: every team width and the cold path,
the rescale on wide and spiked scores, bit-exactness, hand CSR, the model."""
import pytest
import torch

from roc_amd import AdamOptimizer, Trainer, build_model
from roc_amd.ops import functional as F
from roc_amd.ops import reference as ref

from test_gatv2_cpu import loop_gatv2, v2_hand_values
from test_graph_attention_cpu import ATT_ROWS, att_hand_graph
from test_graph_attention_gpu import CASES, DEV, N, _dataset, check, graph

pytestmark = pytest.mark.gpu

_CACHE = {}


def values(heads, dh):
    """bf16-representable fp32 (xl, xr, att, dy) for one shape."""
    key = ("v", heads, dh)
    if key not in _CACHE:
        gen = torch.Generator().manual_seed(100 * heads + dh)
        D = heads * dh
        _CACHE[key] = tuple(
            torch.randn(*s, generator=gen).bfloat16().float().contiguous()
            for s in ((N, D), (N, D), (heads, dh), (N, D)))
    return _CACHE[key]


def reference(xl, xr, att, dy, heads):
    """out, dxl, dxr, datt of the CPU composition in float64."""
    sh, _ = graph()
    xl, xr, att = (t.double().requires_grad_(True) for t in (xl, xr, att))
    out = ref.gatv2_attention(xl, xr, att, sh.rowptr, sh.colidx, N, heads, 0.2)
    out.backward(dy.double())
    return out.detach(), xl.grad, xr.grad, att.grad


def expected(heads, dh):
    key = ("e", heads, dh)
    if key not in _CACHE:
        _CACHE[key] = reference(*values(heads, dh), heads)
    return _CACHE[key]


def run_gpu(xl, xr, att, dy, heads, dtype, backward=True):
    _, shg = graph()
    xlg = xl.to(dtype).to(DEV).requires_grad_(backward)
    xrg = xr.to(dtype).to(DEV).requires_grad_(backward)
    ag = att.to(DEV).requires_grad_(backward)        # fp32 in every case
    out = F.gatv2_attention(xlg, xrg, ag, shg, heads)
    assert out.dtype == dtype and out.shape == xrg.shape
    if not backward:
        return (out.cpu().double(),)
    out.backward(dy.to(dtype).to(DEV))
    assert xlg.grad.dtype == dtype and xrg.grad.dtype == dtype
    assert ag.grad.dtype == torch.float32 and ag.grad.shape == att.shape
    return tuple(t.detach().cpu().double()
                 for t in (out, xlg.grad, xrg.grad, ag.grad))


# datt in bf16. The backward reads the stored bf16 `out` for delta, and datt
# sums that rounding over every edge, so the project's gradient allowance
# (peak * 2^-7 + 1e-2) does not fit it: on the (1, 8) case the kernel is
# 4.144e-01 off the float64 reference at a peak of 37.49 (103% of it). An
# exact fp32 evaluation of the kernels' formulas on the same bf16 inputs
# (out rounded to bf16 before delta, everything else fp32) is 4.145e-01 off
# there, and 0.0015 to 0.0111 of datt's peak over the eight bf16 cases of
# CASES (profiles/r45). Allowed: twice the worst, 0.0222 of the peak.
DATT_BF16 = 2 * 0.0111


def check_all(got, want, dtype):
    for name, g, w in zip(("out", "dxl", "dxr"), got, want):
        check(name, g, w, dtype, name != "out")
    if len(got) < 4:
        return
    if dtype == torch.float32:     # like any gradient, against its own peak
        return check("datt", got[3], want[3], dtype, True)
    err = float((got[3] - want[3]).abs().max())
    peak = float(want[3].abs().max())
    allow = DATT_BF16 * peak
    print(f"datt: max err {err:.3e}, peak {peak:.3e}, allowed {allow:.3e}")
    assert err <= allow, f"datt: {err:.3e} > {allow:.3e}"


@pytest.mark.parametrize("dtype,heads,dh", CASES)
def test_forward_backward(dtype, heads, dh):
    check_all(run_gpu(*values(heads, dh), heads, dtype), expected(heads, dh),
              dtype)


SPIKE_H, SPIKE_DH = 4, 64


def spiked():
    """att scaled by 3 and xl by 2: scores span more than +-100. And one
    source each (xl = 8 * sign(att)) that scores 50 or more above the rest of
    a row at its first edge, at edge 20 (past the first 16) and at its last."""
    if "spike" not in _CACHE:
        sh, _ = graph()
        xl, xr, att, dy = (t.clone() for t in values(SPIKE_H, SPIKE_DH))
        xl, att = 2 * xl, 3 * att
        deg = (sh.rowptr[1:] - sh.rowptr[:-1]).tolist()
        col = sh.colidx.tolist()

        def scores(v):
            """[deg, H] scores of row v"""
            e0 = int(sh.rowptr[v])
            z = (xl[col[e0:e0 + deg[v]]] + xr[v]).view(-1, SPIKE_H, SPIKE_DH)
            return (torch.nn.functional.leaky_relu(z.double(), 0.2)
                    * att.double()).sum(2)

        lo = min(float(scores(v).min()) for v in range(0, N, 7))
        hi = max(float(scores(v).max()) for v in range(0, N, 7))
        assert lo < -100 and hi > 100, (lo, hi)
        rows, taken, seen = [], set(), set()
        for where in ("first", "middle", "last"):
            for v in range(N):
                e0 = int(sh.rowptr[v])
                nbrs = col[e0:e0 + deg[v]]
                pos = {"first": 0, "middle": 20, "last": deg[v] - 1}[where]
                # one spike per chosen row: its source sits in no other one
                if (deg[v] < 29 or taken & set(nbrs) or nbrs[pos] in seen
                        or nbrs.count(nbrs[pos]) != 1):
                    continue
                xl[nbrs[pos]] = 8 * att.sign().reshape(-1)
                taken.add(nbrs[pos])
                seen |= set(nbrs)
                rows.append((v, pos))
                break
        assert len(rows) == 3
        for v, pos in rows:
            s = scores(v)
            gap = s[pos] - torch.cat([s[:pos], s[pos + 1:]]).max(0).values
            assert float(gap.min()) >= 50, (v, pos, gap)
        _CACHE["spike"] = (xl, xr, att, dy,
                           reference(xl, xr, att, dy, SPIKE_H))
    return _CACHE["spike"]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_rescale_on_wide_and_spiked_scores(dtype):
    xl, xr, att, dy, want = spiked()
    fp32 = dtype == torch.float32       # fp32: forward + backward
    got = run_gpu(xl, xr, att, dy, SPIKE_H, dtype, backward=fp32)
    check_all(got, want, dtype)


def _raw(dtype, heads, dh, order, with_lse=True):
    """fwd, bwd_dst and bwd_src through _C with a given row order."""
    from roc_amd import _C
    _, shg = graph()
    xl, xr, att, dy = values(heads, dh)
    xl, xr, dy = (t.to(dtype).to(DEV) for t in (xl, xr, dy))
    att = att.to(DEV)
    fo = to = None
    if order == "reversed":
        fo = torch.arange(N - 1, -1, -1, dtype=torch.int32, device=DEV)
        to = fo.clone()
    out = torch.full_like(xr, 7.0)
    lse = torch.full((N, heads), 7.0, device=DEV) if with_lse else None
    _C.gatv2_attn_fwd(out, lse, xl, xr, att, shg.rowptr, shg.colidx, fo,
                      heads, 0.2)
    if not with_lse:
        return (out,)
    dxr, datt, dxl = (torch.full_like(t, 7.0) for t in (xr, att, xl))
    delta = torch.full_like(lse, 7.0)
    _C.gatv2_attn_bwd_dst(dxr, datt, delta, dy, out, lse, xl, xr, att,
                          shg.rowptr, shg.colidx, fo, heads, 0.2)
    _C.gatv2_attn_bwd_src(dxl, xl, xr, att, dy, lse, delta, shg.t_rowptr,
                          shg.t_colidx, to, heads, 0.2)
    return out, lse, delta, dxr, dxl, datt


@pytest.mark.parametrize("dtype,heads,dh", [(torch.float32, 4, 64),
                                            (torch.bfloat16, 1, 264),
                                            (torch.bfloat16, 4, 64)])
def test_bit_exact_across_calls_and_row_order(dtype, heads, dh):
    a = _raw(dtype, heads, dh, None)
    b = _raw(dtype, heads, dh, None)
    c = _raw(dtype, heads, dh, "reversed")
    for x, y in zip(a, b):              # datt included
        assert torch.equal(x, y)
    for x, z in zip(a[:5], c[:5]):      # per-row outputs only
        assert torch.equal(x, z)
    # another row order regroups datt's fp32 sums: rounding apart, no more
    check("datt", c[5].cpu().double(), a[5].cpu().double(), torch.float32,
          True)
    (no_lse,) = _raw(dtype, heads, dh, None, with_lse=False)
    assert torch.equal(a[0], no_lse)


@pytest.mark.parametrize("dtype,heads,dh", [(torch.float32, 2, 4),
                                            (torch.bfloat16, 2, 8),
                                            (torch.float32, 2, 3)])
def test_hand_csr(dtype, heads, dh):
    from roc_amd import _C
    g = att_hand_graph()
    xl, xr, att, dy = v2_hand_values(heads, dh)
    # On six rows the bf16 rounding of `out` inside delta alone moves dxr by
    # 1.8e-02 at a peak of 0.36 (144% of the allowance, in an fp32 evaluation
    # as in the kernel): the row loop reads `out` as stored, as the op does.
    want = loop_gatv2(xl, xr, att, dy, heads, out_dtype=dtype)
    for name in ("rowptr", "colidx", "t_rowptr", "t_colidx"):
        setattr(g, name, getattr(g, name).to(DEV))
    xlg, xrg = xl.to(dtype).to(DEV), xr.to(dtype).to(DEV)
    ag = att.float().to(DEV)
    out = torch.full_like(xrg, 7.0)         # empty rows must write zeros
    lse = torch.full((g.n_local, heads), 7.0, device=DEV)
    _C.gatv2_attn_fwd(out, lse, xlg, xrg, ag, g.rowptr, g.colidx, None, heads,
                      0.2)
    empty = [v for v, r in enumerate(ATT_ROWS) if not r]
    assert not out[empty].any() and not lse[empty].any()
    for t in (xlg, xrg, ag):
        t.requires_grad_(True)
    o = F.gatv2_attention(xlg, xrg, ag, g, heads)
    o.backward(dy.to(dtype).to(DEV))
    check_all([t.detach().cpu().double()
               for t in (o, xlg.grad, xrg.grad, ag.grad)], want, dtype)
    assert torch.equal(o.detach(), out)
    assert not xrg.grad[empty].any()
    assert not xlg.grad[6].any()            # orphan source


def test_no_edges_returns_zeros():
    n = 5
    z64 = torch.zeros(n + 1, dtype=torch.int64, device=DEV)
    z32 = torch.zeros(0, dtype=torch.int32, device=DEV)
    xl, xr, att = (torch.randn(*s, device=DEV, requires_grad=True)
                   for s in ((n, 16), (n, 16), (2, 8)))
    out = F.gatv2_attention_csr(xl, xr, att, z64, z32, z64, z32, n, n, 2)
    out.backward(torch.ones_like(out))
    assert not out.any() and not xl.grad.any() and not xr.grad.any()
    assert not att.grad.any()


def test_gatv2_fp32_matches_cpu():
    """fp32 logits and every parameter gradient (att included) against the
    CPU model; the last layer (1 head of c = 7 columns) runs the cold path."""
    g, feats, labels, mask, c, shard = _dataset(0.15, 9)
    res = {}
    for dev in ("cpu", DEV):
        model = build_model("gatv2", [feats.shape[1], 64, c], dropout=0.0,
                            seed=1, heads=4)
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


def _bf16_trainer(dropout, capture=False):
    g, feats, labels, mask, c, shard = _dataset(0.2, 7)
    model = build_model("gatv2", [feats.shape[1], 64, c], dropout=dropout,
                        seed=1, heads=4)
    opt = AdamOptimizer(model.parameters(), lr=0.01, weight_decay=1e-4,
                        decay_rate=0.97, decay_steps=100)
    gs = 1.0 / max(int((mask == 1).sum()), 1)
    tr = Trainer(model, shard, feats, labels, mask, opt, device=DEV,
                 compute_dtype=torch.bfloat16, grad_scale=gs, seed=11)
    if capture:
        tr.enable_graph_capture(warmup_epochs=2)
    return tr


def test_gatv2_trains_bf16():
    tr = _bf16_trainer(0.2)
    m0 = tr.evaluate()
    for _ in range(10):
        tr.train_epoch()
    m1 = tr.evaluate()
    assert m1["ce_loss"] == m1["ce_loss"], "NaN loss"
    assert m1["ce_loss"] < m0["ce_loss"], (m0, m1)


def test_gatv2_capture_matches_eager(monkeypatch):
    """Every launch is capturable, the slab allocation included (the
    pattern of tests/test_graph_capture_gpu.py)."""
    monkeypatch.setenv("ROC_DETERMINISTIC", "1")
    tr_e = _bf16_trainer(0.0, capture=True)
    tr_e._graph_warmup = 10 ** 9  # device-schedule eager forever
    for _ in range(8):
        tr_e.train_epoch()
    assert tr_e._graph is None
    tr_g = _bf16_trainer(0.0, capture=True)
    for _ in range(8):
        tr_g.train_epoch()
    captured = tr_g._graph is not None
    F.set_dropout_counter(None)
    assert captured, "graph was never captured"
    for pe, pg in zip((tr_e.model.wl[0], tr_e.model.att[0]),
                      (tr_g.model.wl[0], tr_g.model.att[0])):
        assert torch.allclose(pe.detach().cpu(), pg.detach().cpu(),
                              atol=1e-5), (pe - pg).abs().max()
