"""GATv2 attention on CPU: the index-op reference against a per-row float64
loop on the hand CSR, gradcheck, argument checks, the GATv2 model (single
rank, recompute, ws=2 over gloo) and the train.py flag."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from roc_amd import AdamOptimizer, GATv2, Trainer, build_model, build_shard
from roc_amd.graph import synthetic_dataset, synthetic_graph
from roc_amd.ops import functional as F
from roc_amd.parallel.partition import edge_balanced_bounds

from test_graph_attention_cpu import ATT_NSRC, ATT_ROWS, att_hand_graph

WS = 2
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def v2_hand_values(heads, dh, seed=0):
    """bf16-representable float64 (xl, xr, att, dy) for the hand graph."""
    gen = torch.Generator().manual_seed(seed)
    D = heads * dh
    shapes = ((ATT_NSRC, D), (len(ATT_ROWS), D), (heads, dh),
              (len(ATT_ROWS), D))
    return tuple(torch.randn(*s, generator=gen).bfloat16().double()
                 for s in shapes)


def loop_gatv2(xl, xr, att, dy, heads, slope=0.2, rows=ATT_ROWS,
               out_dtype=None):
    """out, dxl, dxr, datt by a per-row Python loop in float64 (the softmax
    gradient written out: ds = alpha * (dalpha - <dy, out>)). With out_dtype
    the backward reads `out` as stored in that dtype, as the kernels do."""
    xl, xr, att, dy = xl.double(), xr.double(), att.double(), dy.double()
    n, D = xr.shape
    dh = D // heads
    out = torch.zeros(n, D, dtype=torch.float64)
    dxl, dxr, datt = (torch.zeros_like(t) for t in (xl, xr, att))
    for v, nbrs in enumerate(rows):
        for h in range(heads if nbrs else 0):
            c = slice(h * dh, (h + 1) * dh)
            X = torch.stack([xl[u, c] for u in nbrs])
            z = X + xr[v, c]
            a = torch.softmax(torch.where(z > 0, z, slope * z) @ att[h], 0)
            out[v, c] = a @ X
            da = X @ dy[v, c]
            o = out[v, c] if out_dtype is None else \
                out[v, c].to(out_dtype).double()
            ds = a * (da - dy[v, c] @ o)
            dz = ds[:, None] * att[h] * torch.where(z > 0, 1.0, slope)
            dxr[v, c] = dz.sum(0)
            datt[h] += ds @ torch.where(z > 0, z, slope * z)
            for i, u in enumerate(nbrs):
                dxl[u, c] += a[i] * dy[v, c] + dz[i]
    return out, dxl, dxr, datt


@pytest.mark.parametrize("heads,dh", [(1, 4), (2, 3)])
def test_hand_csr_matches_row_loop(heads, dh):
    g = att_hand_graph()
    xl, xr, att, dy = v2_hand_values(heads, dh)
    want = loop_gatv2(xl, xr, att, dy, heads, slope=0.3)
    for t in (xl, xr, att):
        t.requires_grad_(True)
    out = F.gatv2_attention(xl, xr, att, g, heads, slope=0.3)
    assert out.dtype == torch.float64 and out.shape == xr.shape
    out.backward(dy)
    for got, w in zip((out, xl.grad, xr.grad, att.grad), want):
        assert torch.allclose(got, w, atol=1e-12)
    for v in (2, 4):    # empty rows: 0 out, 0 dxr
        assert not out[v].any() and not xr.grad[v].any()
    assert not xl.grad[6].any()                         # orphan source
    assert torch.allclose(out[1], xl[3].detach(), atol=1e-12)   # one edge
    o32 = F.gatv2_attention(*(t.detach().float() for t in (xl, xr, att)), g,
                            heads, slope=0.3)       # fp32 stays fp32
    assert o32.dtype == torch.float32
    assert torch.allclose(o32.double(), want[0], atol=1e-5)


def test_gradcheck_float64():
    sh = build_shard(synthetic_graph(12, 40, seed=2), 0, 1)
    torch.manual_seed(5)
    H, dh = 2, 3
    xl, xr, att = (torch.randn(*s, dtype=torch.float64, requires_grad=True)
                   for s in ((sh.n_ext, H * dh), (sh.n_local, H * dh),
                             (H, dh)))
    assert torch.autograd.gradcheck(
        lambda a, b, c: F.gatv2_attention(a, b, c, sh, H), (xl, xr, att))


def test_shape_and_dtype_checks():
    g = att_hand_graph()
    xl, xr, att, _ = v2_hand_values(2, 4)
    for bad, match in (((xl, xr[:-1], att), "xr must be"),
                       ((xl[:-1], xr, att), "xl must be"),
                       ((xl[:, :-1], xr, att), "xl must be"),
                       ((xl.float(), xr, att), "share a dtype"),
                       ((xl, xr, att[:, :-1]), "att must be"),
                       ((xl.float(), xr.float(), att), "att must be")):
        with pytest.raises(ValueError, match=match):
            F.gatv2_attention(*bad, g, 2)
    with pytest.raises(ValueError, match="heads"):
        F.gatv2_attention(xl, xr, att, g, 3)


def _cora():
    g, feats, labels, mask, c = synthetic_dataset("cora", scale=0.05, seed=3)
    return g, feats, labels, mask, c, build_shard(g, 0, 1)


def _train(sh, feats, labels, mask, c, epochs, heads=2, dropout=0.0,
           recompute=False, **kw):
    model = build_model("gatv2", [feats.shape[1], 16, c], dropout=dropout,
                        seed=1, heads=heads, **kw)
    model.recompute = recompute
    opt = AdamOptimizer(model.parameters(), lr=0.01, weight_decay=1e-4,
                        no_decay=model.norm_parameters())
    tr = Trainer(model, sh, feats, labels, mask, opt, seed=5)
    m0 = tr.evaluate()
    for _ in range(epochs):
        tr.train_epoch()
    return model, m0, tr.evaluate()


@pytest.mark.parametrize("norm", ["none", "layer"])
def test_gatv2_trains_and_every_parameter_gets_gradient(norm):
    torch.manual_seed(0)
    *_, feats, labels, mask, c, sh = _cora()
    model, m0, m1 = _train(sh, feats, labels, mask, c, 10, heads=4,
                           dropout=0.2, norm=norm)
    assert isinstance(model, GATv2) and model.heads == [4, 1]
    assert model.att[0].shape == (4, 4) and model.att[1].shape == (1, c)
    assert np.isfinite(m1["ce_loss"]) and m1["ce_loss"] < m0["ce_loss"]
    assert len(list(model.parameters())) == (8 if norm == "layer" else 6)
    for name, p in model.named_parameters():
        assert p.grad is not None and p.grad.abs().sum() > 0, name
    with pytest.raises(AssertionError, match="not divisible by 4 heads"):
        GATv2([10, 6, 3], heads=4)


def test_gatv2_recompute_matches_standard():
    torch.manual_seed(0)
    *_, feats, labels, mask, c, sh = _cora()
    a, b = (_train(sh, feats, labels, mask, c, 2, dropout=0.3,
                   recompute=rec)[0] for rec in (False, True))
    for pa, pb in zip(a.parameters(), b.parameters()):
        assert torch.allclose(pa, pb, atol=1e-6)


def _ws2_worker(rank, port, q):
    try:
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        os.environ["ROC_COMM_MODE"] = "halo"
        dist.init_process_group("gloo", rank=rank, world_size=WS)
        torch.manual_seed(0)
        g, feats, labels, mask, c = synthetic_dataset("cora", scale=0.05,
                                                      seed=3)
        sh = build_shard(g, rank, WS, edge_balanced_bounds(g.rowptr, WS))
        model, _, md = _train(sh, feats, labels, mask, c, 3)
        q.put((rank, md, [p.detach().numpy().copy()
                          for p in (model.wl[0], model.att[0])], None))
    except Exception:  # pragma: no cover
        import traceback
        q.put((rank, None, None, traceback.format_exc()))
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()


def test_gatv2_ws2_matches_single_rank():
    ctx = mp.get_context("spawn")
    q = ctx.SimpleQueue()
    procs = [ctx.Process(target=_ws2_worker, args=(r, 29587, q))
             for r in range(WS)]
    for p in procs:
        p.start()
    res = sorted([q.get() for _ in range(WS)], key=lambda t: t[0])
    for p in procs:
        p.join(timeout=180)
    for rank, md, w, err in res:
        assert err is None, f"rank {rank}: {err}"
    torch.manual_seed(0)
    *_, feats, labels, mask, c, sh = _cora()
    model, _, md1 = _train(sh, feats, labels, mask, c, 3)
    for k, p in enumerate((model.wl[0], model.att[0])):
        w0 = torch.from_numpy(res[0][2][k])
        assert torch.allclose(w0, torch.from_numpy(res[1][2][k]), atol=1e-6)
        assert torch.allclose(p.detach(), w0, atol=1e-4), \
            (p.detach() - w0).abs().max()
    assert res[0][1]["train_total"] == md1["train_total"]
    assert abs(res[0][1]["ce_loss"] - md1["ce_loss"]) < 1e-3


def test_cli_model_gatv2():
    env = {k: v for k, v in os.environ.items()
           if k not in ("RANK", "WORLD_SIZE")}
    env["CUDA_VISIBLE_DEVICES"] = ""
    env["HIP_VISIBLE_DEVICES"] = ""
    r = subprocess.run(
        [sys.executable, os.path.join(REPO, "train.py"), "--model", "gatv2",
         "--scale", "0.05", "--epochs", "3", "--eval-every", "1", "--norm",
         "layer", "--heads", "2"],
        capture_output=True, text=True, timeout=300, env=env, cwd=REPO)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "model=gatv2" in r.stdout
    lines = [l for l in r.stdout.splitlines() if l.startswith("epoch")]
    assert len(lines) == 3, r.stdout
