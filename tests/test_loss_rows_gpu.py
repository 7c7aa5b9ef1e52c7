"""The loss-row-pruned transpose plan must not change a single bit.

An edge whose column's operand row is zero adds +-0 to an fp32 sum that
starts at +0, so the strip SpMM over the pruned plan equals the one over
the full plan (``torch.equal``) on any dy that is zero on the dropped
rows, and a GCN trained with the plan has the weights of one trained
without it.

Graph: 3001 nodes, lognormal in-degree (hub rows far above the heavy
threshold of 24 in one 256-wide window), window 256: 12 strips of the full
plan, and most rows have empty segments."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from roc_amd import AdamOptimizer, Trainer, build_model
from roc_amd.graph import synthetic_graph, MASK_TRAIN, MASK_VAL
from roc_amd.ops import functional as F
from roc_amd.parallel import partition
from roc_amd.parallel.partition import (build_loss_strip_plan, build_shard,
                                        build_strip_heavy, build_strip_plan)

DEV = "cuda:0"
N, E, WIDTH, HEAVY_MIN = 3001, 60000, 256, 24
DIMS = [16, 64, 256]  # TEAM 8 (partly idle), TEAM 8, TEAM 32
FRACS = [0.0, 0.7, 1.0]


def _dev(strips):
    return [(a.to(DEV), b.to(DEV)) for a, b in strips]


@pytest.fixture(scope="module")
def setup():
    # any sorted CSR serves as "the transpose": the skewed forward CSR has
    # the heavy rows
    g = synthetic_graph(N, E, seed=4, skew=1.5)
    rp, ci = g.rowptr, g.colidx.to(torch.int32)
    full = build_strip_plan(rp, ci, N, WIDTH)
    heavy = build_strip_heavy(full, HEAVY_MIN)
    assert len(full) == 12 and sum(h.numel() for h in heavy) >= 3
    seg = np.stack([np.diff(srp.numpy()) for srp, _ in full])
    assert (seg == 0).any()  # empty strip segments
    gen = torch.Generator().manual_seed(3)
    u = torch.rand(N, generator=gen)
    plans = {}
    for frac in FRACS:
        keep = u < frac
        strips, _ = build_loss_strip_plan(rp, ci, keep, WIDTH)
        plans[frac] = (keep.to(DEV), _dev(strips),
                       [h.to(DEV) for h in build_strip_heavy(strips,
                                                             HEAVY_MIN)])
    assert len(plans[0.0][1]) == 1 and len(plans[1.0][1]) == 12
    assert 8 <= len(plans[0.7][1]) <= 9
    dys = {D: torch.randn(N, D, generator=gen).to(torch.bfloat16).to(DEV)
           for D in DIMS}
    return _dev(full), [h.to(DEV) for h in heavy], plans, dys


@pytest.mark.parametrize("frac", FRACS)
@pytest.mark.parametrize("D", DIMS)
def test_pruned_backward_bit_equal(setup, D, frac):
    full, heavy, plans, dys = setup
    keep, strips, lheavy = plans[frac]
    dy = dys[D] * keep.unsqueeze(1).to(torch.bfloat16)
    if frac == 0.7:  # a dead row of -0 is as dead as one of +0
        dead = (~keep).nonzero()[:5, 0]
        dy[dead] = -0.0
    want = F._strip_spmm(dy, full, N, None, heavy, HEAVY_MIN)
    got = F._strip_spmm(dy, strips, N, None, lheavy, HEAVY_MIN)
    assert torch.equal(got, want)
    if frac == 0.0:
        assert not got.any()


def _shard(g, mask, on, monkeypatch):
    monkeypatch.setenv("ROC_SPMM_STRIP_MIN_EDGES", "1")
    monkeypatch.setenv("ROC_SPMM_STRIP_WIDTH", str(WIDTH))
    monkeypatch.setattr(partition, "_HEAVY_MIN", 4)
    monkeypatch.setattr(partition, "_LOSS_ROWS", (on, WIDTH))
    sh = build_shard(g, 0, 1)
    assert sh.bwd_strips is not None and sh.bwd_strip_order is None
    return sh


def _mask(n, seed=9):
    u = torch.rand(n, generator=torch.Generator().manual_seed(seed))
    mask = torch.full((n,), MASK_TRAIN, dtype=torch.int32)
    mask[u >= 0.7] = MASK_VAL
    return mask


def test_debug_switch_raises_on_a_nonzero_dead_row(monkeypatch):
    g = synthetic_graph(N, E, seed=4, skew=1.5)
    mask = _mask(N)
    sh = _shard(g, mask, True, monkeypatch)
    assert sh.install_loss_rows(mask == MASK_TRAIN)
    sh = sh.to(DEV)
    monkeypatch.setattr(F, "_DEBUG_LOSS_ROWS", True)
    gen = torch.Generator().manual_seed(1)
    x = torch.randn(N, 16, generator=gen).to(torch.bfloat16).to(DEV)
    dy = torch.randn(N, 16, generator=gen).to(torch.bfloat16).to(DEV)
    dy = dy * (mask == MASK_TRAIN).to(DEV).unsqueeze(1).to(torch.bfloat16)
    for bad in (False, True):
        xg = x.clone().requires_grad_()
        out = F.scatter_gather(xg, sh, loss_rows_only=True)
        d = dy.clone()
        if bad:
            d[int((mask != MASK_TRAIN).nonzero()[7]), 3] = 1.0
            with pytest.raises(RuntimeError, match="loss_rows_only"):
                out.backward(d)
        else:
            out.backward(d)
            full = x.clone().requires_grad_()
            F.scatter_gather(full, sh).backward(d)
            assert torch.equal(xg.grad, full.grad)


# 24 -> 32 widens, so layer 0 aggregates first and applies its ReLU as a pass
# of its own; 32 -> 32 is the benchmark's shape of layer: linear first, the
# ReLU in the SpMM's store, the backward scaling handed to the transpose SpMM
@pytest.mark.parametrize("dims", [[24, 32, 16], [32, 32, 16]])
@pytest.mark.parametrize("capture", [False, True])
def test_trained_weights_bit_equal(monkeypatch, capture, dims):
    """3 epochs of a 2-layer GCN with the plan and without
    (ROC_SPMM_LOSS_ROWS=0), eager and under graph capture. Eager is not
    compared with capture: a captured epoch takes its Adam step size and
    dropout offsets from a device counter, which the optimizer's own test
    holds to 1e-6 of the host schedule, not to the bit."""
    g = synthetic_graph(N, E, seed=4, skew=1.5)
    gen = torch.Generator().manual_seed(2)
    feats = torch.randn(N, dims[0], generator=gen)
    labels = torch.randint(0, 16, (N,), generator=gen)
    mask = _mask(N)
    got = {}
    for on in (False, True):
        sh = _shard(g, mask, on, monkeypatch)
        model = build_model("gcn", dims, dropout=0.5, seed=1)
        opt = AdamOptimizer(model.parameters(), lr=0.01, weight_decay=1e-4)
        tr = Trainer(model, sh, feats, labels, mask, opt, device=DEV,
                     compute_dtype=torch.bfloat16, seed=1)
        assert (tr.shard.bwd_loss_strips is not None) == on
        if capture:
            tr.enable_graph_capture(warmup_epochs=1)
        for _ in range(3):
            tr.train_epoch()
        tr.sync()
        assert not capture or tr._graph is not None
        got[on] = [w.detach().clone() for w in model.weights]
    for a, b in zip(got[False], got[True]):
        assert torch.equal(a, b)
    assert not torch.equal(
        got[True][0].cpu(),
        build_model("gcn", dims, seed=1).weights[0].detach())
