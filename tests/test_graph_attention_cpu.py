"""Dot-product graph attention on CPU: the index-op reference against a
per-row float64 loop and against the existing edge ops, invariances,
gradcheck, the GraphTransformer model (single rank, ws=2 over gloo) and
the train.py flag."""
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from roc_amd import (AdamOptimizer, GraphTransformer, Trainer, build_model,
                     build_shard)
from roc_amd.graph import build_transpose, synthetic_dataset, synthetic_graph
from roc_amd.ops import functional as F
from roc_amd.ops import reference as ref
from roc_amd.parallel.partition import edge_balanced_bounds

WS = 2
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# in-neighbor lists of the hand-built graph (6 rows, 7 sources)
ATT_ROWS = [
    [0, 1, 0],      # a duplicate edge (source 0 twice)
    [3],            # a one-edge row: alpha = 1
    [],             # empty row
    [2, 4, 5, 1],
    [],             # a second empty row
    [5, 5, 3],      # a duplicate again, on another source
]
ATT_NSRC = 7        # source 6 has no out-edge: its dkv row is zero


def att_hand_graph():
    rowptr = torch.tensor(np.cumsum([0] + [len(r) for r in ATT_ROWS]),
                          dtype=torch.int64)
    colidx = torch.tensor([u for r in ATT_ROWS for u in r], dtype=torch.int32)
    t_rowptr, t_colidx = build_transpose(ATT_NSRC, rowptr, colidx)
    return SimpleNamespace(rowptr=rowptr, colidx=colidx, t_rowptr=t_rowptr,
                           t_colidx=t_colidx, n_local=len(ATT_ROWS),
                           n_ext=ATT_NSRC, row_order=None, t_row_order=None)


def att_hand_values(heads, dh, seed=0):
    """bf16-representable float64 (q, kv, dy) for the hand graph."""
    gen = torch.Generator().manual_seed(seed)
    D = heads * dh
    q = torch.randn(len(ATT_ROWS), D, generator=gen)
    kv = torch.randn(ATT_NSRC, 2 * D, generator=gen)
    dy = torch.randn(len(ATT_ROWS), D, generator=gen)
    return tuple(t.bfloat16().double() for t in (q, kv, dy))


def loop_attention(q, kv, dy, heads, scale=None, rows=ATT_ROWS):
    """out, dq, dkv by a per-row Python loop in float64 (the softmax
    gradient written out: ds = alpha * (dalpha - <alpha, dalpha>))."""
    q, kv, dy = q.double(), kv.double(), dy.double()
    n, D = q.shape
    dh = D // heads
    scale = dh ** -0.5 if scale is None else scale
    out = torch.zeros(n, D, dtype=torch.float64)
    dq = torch.zeros_like(q)
    dkv = torch.zeros_like(kv)
    for v, nbrs in enumerate(rows):
        if not nbrs:
            continue
        for h in range(heads):
            c = slice(h * dh, (h + 1) * dh)
            cv = slice(D + h * dh, D + (h + 1) * dh)
            K = torch.stack([kv[u, c] for u in nbrs])
            V = torch.stack([kv[u, cv] for u in nbrs])
            s = scale * (K @ q[v, c])
            a = torch.softmax(s, 0)
            out[v, c] = a @ V
            da = V @ dy[v, c]
            ds = a * (da - (a * da).sum())
            dq[v, c] = scale * (ds @ K)
            for i, u in enumerate(nbrs):
                dkv[u, c] += scale * ds[i] * q[v, c]
                dkv[u, cv] += a[i] * dy[v, c]
    return out, dq, dkv


@pytest.mark.parametrize("heads,dh", [(1, 4), (2, 3)])
def test_hand_csr_matches_row_loop(heads, dh):
    g = att_hand_graph()
    q, kv, dy = att_hand_values(heads, dh)
    want_out, want_dq, want_dkv = loop_attention(q, kv, dy, heads)
    q.requires_grad_(True)
    kv.requires_grad_(True)
    out = F.graph_attention(q, kv, g, heads)
    assert out.dtype == torch.float64 and out.shape == q.shape
    out.backward(dy)
    assert torch.allclose(out, want_out, atol=1e-12)
    assert torch.allclose(q.grad, want_dq, atol=1e-12)
    assert torch.allclose(kv.grad, want_dkv, atol=1e-12)
    for v in (2, 4):    # empty rows: 0 out, 0 dq
        assert torch.equal(out[v], torch.zeros_like(out[v]))
        assert torch.equal(q.grad[v], torch.zeros_like(q.grad[v]))
    assert torch.equal(kv.grad[6], torch.zeros_like(kv.grad[6]))  # orphan
    # the one-edge row copies V of its source
    D = heads * dh
    assert torch.allclose(out[1], kv[3, D:].detach(), atol=1e-12)


def test_explicit_scale_and_fp32():
    g = att_hand_graph()
    q, kv, dy = att_hand_values(2, 4, seed=1)
    want, _, _ = loop_attention(q, kv, dy, 2, scale=0.3)
    out = F.graph_attention(q.float(), kv.float(), g, 2, scale=0.3)
    assert out.dtype == torch.float32
    assert torch.allclose(out.double(), want, atol=1e-5)
    out2 = F.graph_attention_csr(q.float(), kv.float(), g.rowptr, g.colidx,
                                 g.t_rowptr, g.t_colidx, g.n_local, g.n_ext,
                                 2, scale=0.3)
    assert torch.equal(out, out2)


def _cora():
    g, feats, labels, mask, c = synthetic_dataset("cora", scale=0.05, seed=3)
    return g, feats, labels, mask, c, build_shard(g, 0, 1)


def test_matches_existing_edge_ops():
    """H = 1: the fused op equals edge_dot -> edge_softmax ->
    scatter_gather_weighted, forward and gradients."""
    torch.manual_seed(2)
    *_, sh = _cora()
    D = 8
    scale = D ** -0.5
    q1 = torch.randn(sh.n_local, D, requires_grad=True)
    kv1 = torch.randn(sh.n_ext, 2 * D, requires_grad=True)
    q2 = q1.detach().clone().requires_grad_(True)
    kv2 = kv1.detach().clone().requires_grad_(True)
    dy = torch.randn(sh.n_local, D)
    out = F.graph_attention(q1, kv1, sh, 1)
    out.backward(dy)
    K, V = kv2[:, :D].contiguous(), kv2[:, D:].contiguous()
    # edge_dot(dy, x) = <dy[row_e], x[col_e]>: q rides the row side
    alpha = F.edge_softmax(scale * ref.edge_dot(q2, K, sh.rowptr, sh.colidx),
                           sh)
    want = F.scatter_gather_weighted(V, alpha, sh)
    want.backward(dy)
    assert torch.allclose(out, want, atol=1e-5), (out - want).abs().max()
    assert torch.allclose(q1.grad, q2.grad, atol=1e-5)
    assert torch.allclose(kv1.grad, kv2.grad, atol=1e-5)


def test_constant_v_gives_ones():
    torch.manual_seed(3)
    *_, sh = _cora()
    D, H = 12, 3
    q = torch.randn(sh.n_local, D)
    kv = torch.cat([torch.randn(sh.n_ext, D), torch.ones(sh.n_ext, D)], 1)
    out = F.graph_attention(q, kv, sh, H)
    deg = sh.rowptr[1:] - sh.rowptr[:-1]
    assert int((deg > 0).sum()) > 0
    assert torch.allclose(out[deg > 0], torch.ones(int((deg > 0).sum()), D),
                          atol=1e-6)
    assert torch.equal(out[deg == 0], torch.zeros(int((deg == 0).sum()), D))


def test_constant_k_shift_leaves_out_unchanged():
    torch.manual_seed(4)
    *_, sh = _cora()
    D, H = 12, 2
    q = torch.randn(sh.n_local, D, dtype=torch.float64)
    kv = torch.randn(sh.n_ext, 2 * D, dtype=torch.float64)
    shift = torch.zeros(2 * D, dtype=torch.float64)
    shift[:D] = torch.randn(D, dtype=torch.float64)
    a = F.graph_attention(q, kv, sh, H)
    b = F.graph_attention(q, kv + shift, sh, H)
    assert torch.allclose(a, b, atol=1e-9), (a - b).abs().max()


def test_gradcheck_float64():
    g = synthetic_graph(12, 40, seed=2)
    sh = build_shard(g, 0, 1)
    torch.manual_seed(5)
    H, dh = 2, 3
    q = torch.randn(sh.n_local, H * dh, dtype=torch.float64,
                    requires_grad=True)
    kv = torch.randn(sh.n_ext, 2 * H * dh, dtype=torch.float64,
                     requires_grad=True)
    assert torch.autograd.gradcheck(
        lambda a, b: F.graph_attention(a, b, sh, H), (q, kv))


def test_shape_and_dtype_checks():
    g = att_hand_graph()
    q, kv, _ = att_hand_values(2, 4)
    with pytest.raises(ValueError, match="q must be"):
        F.graph_attention(q[:-1], kv, g, 2)
    with pytest.raises(ValueError, match="kv must be"):
        F.graph_attention(q, kv[:-1], g, 2)
    with pytest.raises(ValueError, match="kv must be"):
        F.graph_attention(q, kv[:, :-1], g, 2)
    with pytest.raises(ValueError, match="heads"):
        F.graph_attention(q, kv, g, 3)
    with pytest.raises(ValueError, match="dtype"):
        F.graph_attention(q.float(), kv, g, 2)


def test_empty_graph_returns_zeros():
    n = 5
    g = SimpleNamespace(rowptr=torch.zeros(n + 1, dtype=torch.int64),
                        colidx=torch.zeros(0, dtype=torch.int32),
                        t_rowptr=torch.zeros(n + 1, dtype=torch.int64),
                        t_colidx=torch.zeros(0, dtype=torch.int32),
                        n_local=n, n_ext=n, row_order=None, t_row_order=None)
    out = F.graph_attention(torch.randn(n, 8), torch.randn(n, 16), g, 2)
    assert torch.equal(out, torch.zeros(n, 8))


# ---------------------------------------------------------------------------
# model
# ---------------------------------------------------------------------------

def _params(model):
    return list(model.wq) + list(model.wkv) + list(model.wskip)


def test_transformer_trains_and_every_parameter_gets_gradient():
    torch.manual_seed(0)
    g, feats, labels, mask, c, sh = _cora()
    model = build_model("transformer", [feats.shape[1], 16, c], dropout=0.2,
                        seed=1, heads=4)
    assert isinstance(model, GraphTransformer)
    assert model.heads == [4, 1]
    assert model.wkv[0].shape == (feats.shape[1], 32)
    opt = AdamOptimizer(model.parameters(), lr=0.01, weight_decay=1e-4)
    tr = Trainer(model, sh, feats, labels, mask, opt)
    m0 = tr.evaluate()
    for _ in range(10):
        tr.train_epoch()
    m1 = tr.evaluate()
    assert np.isfinite(m1["ce_loss"]) and m1["ce_loss"] < m0["ce_loss"]
    for p in _params(model):
        assert p.grad is not None and p.grad.abs().sum() > 0


def test_transformer_init_and_head_assert():
    a = GraphTransformer([10, 8, 3], seed=7, heads=2)
    b = GraphTransformer([10, 8, 3], seed=7, heads=2, norm="layer")
    for pa, pb in zip(_params(a), _params(b)):
        assert torch.equal(pa, pb)  # the norm draws no RNG
    assert [n for n, _ in b.named_parameters() if n.startswith("norm_")] == \
        ["norm_gamma.0", "norm_beta.0"]
    assert a.norm_parameters() == []
    # K and V halves are separate Glorot draws over (in, out)
    assert torch.equal(a.wkv[0][:, :8],
                       ref.glorot_uniform((10, 8), seed=7 + 1))
    assert torch.equal(a.wkv[0][:, 8:],
                       ref.glorot_uniform((10, 8), seed=7 + 2))
    assert torch.equal(a.wskip[1], ref.glorot_uniform((8, 3), seed=7 + 7))
    with pytest.raises(AssertionError, match="not divisible by 4 heads"):
        GraphTransformer([10, 6, 3], heads=4)


def test_transformer_recompute_matches_standard():
    torch.manual_seed(0)
    g, feats, labels, mask, c, sh = _cora()

    def run(rec):
        model = build_model("transformer", [feats.shape[1], 16, c],
                            dropout=0.3, seed=1, heads=2)
        model.recompute = rec
        opt = AdamOptimizer(model.parameters(), lr=0.01)
        tr = Trainer(model, sh, feats, labels, mask, opt, seed=5)
        for _ in range(2):
            tr.train_epoch()
        return model.wq[0].detach()

    assert torch.allclose(run(False), run(True), atol=1e-6)


def test_transformer_layer_norm_runs():
    torch.manual_seed(0)
    g, feats, labels, mask, c, sh = _cora()
    model = build_model("transformer", [feats.shape[1], 16, c], dropout=0.1,
                        seed=1, heads=4, norm="layer")
    opt = AdamOptimizer(model.parameters(), lr=0.01,
                        no_decay=model.norm_parameters())
    tr = Trainer(model, sh, feats, labels, mask, opt)
    for _ in range(3):
        tr.train_epoch()
    assert np.isfinite(tr.evaluate()["ce_loss"])
    assert not torch.equal(model.norm_gamma[0].detach(), torch.ones(16))


def _ws2_worker(rank, port, q):
    try:
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        os.environ["ROC_COMM_MODE"] = "halo"
        dist.init_process_group("gloo", rank=rank, world_size=WS)
        torch.manual_seed(0)
        g, feats, labels, mask, c = synthetic_dataset("cora", scale=0.05,
                                                      seed=3)
        bounds = edge_balanced_bounds(g.rowptr, WS)
        sh = build_shard(g, rank, WS, bounds)
        model = build_model("transformer", [feats.shape[1], 16, c],
                            dropout=0.0, seed=1, heads=2)
        opt = AdamOptimizer(model.parameters(), lr=0.01, weight_decay=1e-4)
        tr = Trainer(model, sh, feats, labels, mask, opt)
        for _ in range(3):
            tr.train_epoch()
        md = tr.evaluate()
        q.put((rank, md, model.wkv[0].detach().numpy().copy(), None))
    except Exception:  # pragma: no cover
        import traceback
        q.put((rank, None, None, traceback.format_exc()))
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()


def test_transformer_ws2_matches_single_rank():
    ctx = mp.get_context("spawn")
    q = ctx.SimpleQueue()
    procs = [ctx.Process(target=_ws2_worker, args=(r, 29583, q))
             for r in range(WS)]
    for p in procs:
        p.start()
    res = sorted([q.get() for _ in range(WS)], key=lambda t: t[0])
    for p in procs:
        p.join(timeout=180)
    for rank, md, w, err in res:
        assert err is None, f"rank {rank}: {err}"
    w0 = torch.from_numpy(res[0][2])
    assert torch.allclose(w0, torch.from_numpy(res[1][2]), atol=1e-6)
    # single-rank baseline
    torch.manual_seed(0)
    g, feats, labels, mask, c = synthetic_dataset("cora", scale=0.05, seed=3)
    sh = build_shard(g, 0, 1)
    model = build_model("transformer", [feats.shape[1], 16, c], dropout=0.0,
                        seed=1, heads=2)
    opt = AdamOptimizer(model.parameters(), lr=0.01, weight_decay=1e-4)
    tr = Trainer(model, sh, feats, labels, mask, opt)
    for _ in range(3):
        tr.train_epoch()
    md1 = tr.evaluate()
    assert torch.allclose(model.wkv[0].detach(), w0, atol=1e-4), \
        (model.wkv[0].detach() - w0).abs().max()
    assert res[0][1]["train_total"] == md1["train_total"]
    assert abs(res[0][1]["ce_loss"] - md1["ce_loss"]) < 1e-3


def test_cli_model_transformer():
    env = dict(os.environ)
    env.pop("RANK", None)
    env.pop("WORLD_SIZE", None)
    env["CUDA_VISIBLE_DEVICES"] = ""
    env["HIP_VISIBLE_DEVICES"] = ""
    r = subprocess.run(
        [sys.executable, os.path.join(REPO, "train.py"), "--model",
         "transformer", "--scale", "0.05", "--epochs", "3", "--eval-every",
         "1", "--norm", "layer"],
        capture_output=True, text=True, timeout=300, env=env, cwd=REPO)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "model=transformer" in r.stdout
    lines = [l for l in r.stdout.splitlines() if l.startswith("epoch")]
    assert len(lines) == 3, r.stdout
    r = subprocess.run(
        [sys.executable, os.path.join(REPO, "train.py"), "--model",
         "transformer", "--scale", "0.05", "--epochs", "3"],
        capture_output=True, text=True, timeout=300, env=env, cwd=REPO)
    assert r.returncode == 0, r.stderr[-2000:]
