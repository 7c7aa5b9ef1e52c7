"""The loss-row-pruned transpose strip plan (partition.build_loss_strip_plan).

A transpose SpMM over it must add exactly the edges whose column is kept,
in their original order, whatever the keep-vector looks like; windows are
cut every `width` kept columns."""
import numpy as np
import pytest
import torch

from roc_amd.graph import synthetic_graph, MASK_TRAIN
from roc_amd.ops import functional as F
from roc_amd.parallel import partition
from roc_amd.parallel.partition import (build_loss_strip_plan, build_shard,
                                        build_strip_heavy, build_strip_plan)

N, WIDTH = 700, 64


@pytest.fixture(scope="module")
def csr():
    g = synthetic_graph(N, 9000, seed=3, skew=1.5)
    sh = build_shard(g, 0, 1)
    return sh.t_rowptr, sh.t_colidx


def _keeps():
    rng = np.random.default_rng(7)
    runs = np.ones(N, dtype=bool)
    runs[40:400] = False      # a dead run of several windows
    runs[401:650:2] = False   # and every other column after it
    return {
        "all": np.ones(N, dtype=bool),
        "none": np.zeros(N, dtype=bool),
        "random": rng.random(N) < 0.7,
        "runs": runs,
    }


def _segments(strips, row):
    return np.concatenate(
        [sci.numpy()[int(srp[row]):int(srp[row + 1])] for srp, sci in strips])


@pytest.mark.parametrize("name", ["all", "none", "random", "runs"])
def test_segments_are_the_kept_edges_in_order(csr, name):
    rp, ci = csr
    keep = _keeps()[name]
    strips, bounds = build_loss_strip_plan(rp, ci, torch.from_numpy(keep),
                                           WIDTH)
    rpn, cin = rp.numpy(), ci.numpy()
    for srp, sci in strips:
        assert srp.dtype == torch.int64 and sci.dtype == ci.dtype
        assert srp.numel() == rp.numel()
    for row in range(rpn.shape[0] - 1):
        edges = cin[rpn[row]:rpn[row + 1]]
        assert np.array_equal(_segments(strips, row), edges[keep[edges]])


@pytest.mark.parametrize("name", ["all", "random", "runs"])
def test_windows_hold_width_live_columns(csr, name):
    rp, ci = csr
    keep = _keeps()[name]
    strips, bounds = build_loss_strip_plan(rp, ci, torch.from_numpy(keep),
                                           WIDTH)
    b = bounds.numpy()
    n_keep = int(keep.sum())
    assert len(strips) == -(-n_keep // WIDTH) == b.shape[0] - 1
    assert b[0] == 0 and b[-1] == N and (np.diff(b) > 0).all()
    for s, (srp, sci) in enumerate(strips):
        c = sci.numpy()
        assert ((c >= b[s]) & (c < b[s + 1])).all()
        live = int(keep[b[s]:b[s + 1]].sum())
        assert live == (WIDTH if s < len(strips) - 1
                        else n_keep - WIDTH * (len(strips) - 1))


def test_keep_all_is_the_ordinary_plan(csr):
    rp, ci = csr
    strips, _ = build_loss_strip_plan(rp, ci, torch.ones(N, dtype=torch.bool),
                                      WIDTH)
    want = build_strip_plan(rp, ci, N, WIDTH)
    assert len(strips) == len(want)
    for (a, b), (c, d) in zip(strips, want):
        assert torch.equal(a, c) and torch.equal(b, d)


def test_keep_none_is_one_empty_strip(csr):
    rp, ci = csr
    strips, bounds = build_loss_strip_plan(
        rp, ci, torch.zeros(N, dtype=torch.bool), WIDTH)
    assert len(strips) == 1 and bounds.tolist() == [0, N]
    srp, sci = strips[0]
    assert sci.numel() == 0 and not srp.any() and srp.numel() == rp.numel()


def test_install_on_shard(monkeypatch):
    """install_loss_rows: heavy lists are build_strip_heavy's on the same
    strips; nothing is built without the ordinary backward plan, or when
    the feature is switched off."""
    g = synthetic_graph(N, 9000, seed=3, skew=1.5)
    keep = torch.from_numpy(_keeps()["random"])
    monkeypatch.setattr(partition, "_LOSS_ROWS", (True, WIDTH))
    plain = build_shard(g, 0, 1)
    assert plain.bwd_strips is None
    assert not plain.install_loss_rows(keep) and plain.bwd_loss_strips is None
    monkeypatch.setenv("ROC_SPMM_STRIP_MIN_EDGES", "1")
    monkeypatch.setenv("ROC_SPMM_STRIP_WIDTH", str(WIDTH))
    monkeypatch.setattr(partition, "_HEAVY_MIN", 3)
    sh = build_shard(g, 0, 1)
    assert sh.bwd_strips is not None and sh.bwd_strip_order is None
    assert sh.install_loss_rows(keep)
    want, _ = build_loss_strip_plan(sh.t_rowptr, sh.t_colidx, keep, WIDTH)
    heavy = build_strip_heavy(want, 3)
    assert any(h.numel() for h in heavy)
    assert len(sh.bwd_loss_heavy) == len(heavy) == len(sh.bwd_loss_strips)
    for a, b in zip(sh.bwd_loss_heavy, heavy):
        assert torch.equal(a, b)
    assert torch.equal(sh.loss_keep, keep)
    monkeypatch.setattr(partition, "_LOSS_ROWS", (False, WIDTH))
    assert not sh.install_loss_rows(keep) and sh.bwd_loss_strips is None


def test_cpu_path_ignores_the_keywords_gradient_unchanged():
    """On the CPU reference path loss_rows_only changes nothing, and
    grad_src_scale with linear(grad_prescaled=True) is the same gradient
    as the linear scaling it itself."""
    g = synthetic_graph(300, 3000, seed=5)
    sh = build_shard(g, 0, 1)
    gen = torch.Generator().manual_seed(1)
    x0 = torch.randn(300, 12, generator=gen)
    w0 = torch.randn(12, 8, generator=gen)
    dy = torch.randn(300, 8, generator=gen)
    dy[torch.rand(300, generator=gen) > 0.7] = 0
    rs = sh.rsqrt_deg_local
    grads = []
    for fuse, loss in ((False, False), (True, True)):
        x = x0.clone().requires_grad_()
        w = w0.clone().requires_grad_()
        h = F.linear(x, w, row_scale=rs, grad_prescaled=fuse)
        out = F.scatter_gather(h, sh, dst_scale=rs, relu=True,
                               grad_src_scale=rs if fuse else None,
                               loss_rows_only=loss)
        out.backward(dy)
        grads.append((out.detach(), x.grad, w.grad))
    for a, b in zip(*grads):
        assert torch.equal(a, b)
    # and relu=True is scatter_gather followed by relu
    x = x0.clone().requires_grad_()
    w = w0.clone().requires_grad_()
    out = F.relu(F.scatter_gather(F.linear(x, w, row_scale=rs), sh,
                                  dst_scale=rs))
    out.backward(dy)
    assert torch.equal(out.detach(), grads[0][0])
    assert torch.equal(x.grad, grads[0][1])
    assert torch.equal(w.grad, grads[0][2])
