"""Heavy-first lists of the strip plans (CPU side: what the strip kernel
is handed must be exactly the rows at or above the threshold, longest
first, and must travel with the shard)."""
import numpy as np
import torch

from roc_amd.graph import synthetic_graph
from roc_amd.parallel import partition
from roc_amd.parallel.partition import (build_shard, build_strip_heavy,
                                        build_strip_plan)


def test_heavy_lists_match_threshold_and_order():
    g = synthetic_graph(2000, 40000, seed=4)
    strips = build_strip_plan(g.rowptr, g.colidx, g.num_nodes, 500)
    for hmin in (0, 1, 12, 10 ** 6):
        heavy = build_strip_heavy(strips, hmin)
        assert len(heavy) == len(strips)
        for (srp, _), h in zip(strips, heavy):
            seg = np.diff(srp.numpy())
            assert h.dtype == torch.int32
            rows = h.numpy()
            assert sorted(rows.tolist()) == np.nonzero(seg >= hmin)[0].tolist()
            assert (np.diff(seg[rows]) <= 0).all()  # longest first
    assert all(h.numel() == 0 for h in build_strip_heavy(strips, 10 ** 6))


def test_shard_carries_heavy_lists(monkeypatch):
    g = synthetic_graph(2000, 40000, seed=4)
    monkeypatch.setenv("ROC_SPMM_STRIP_MIN_EDGES", "0")
    monkeypatch.setenv("ROC_SPMM_STRIP_WIDTH", "500")
    monkeypatch.setattr(partition, "_HEAVY_MIN", 12)
    sh = build_shard(g, 0, 1)
    assert sh.strip_heavy_min == 12
    assert len(sh.fwd_strip_heavy) == len(sh.fwd_strips) == 4
    assert len(sh.bwd_strip_heavy) == len(sh.bwd_strips)
    # the plans stay lists of (rowptr, colidx) pairs
    for srp, sci in sh.fwd_strips:
        assert srp.numel() == g.num_nodes + 1
    moved = sh.to("cpu")
    assert moved.strip_heavy_min == 12
    assert all(torch.equal(a, b) for a, b in
               zip(moved.fwd_strip_heavy, sh.fwd_strip_heavy))
    # knob 0: no lists, natural sweep only
    monkeypatch.setattr(partition, "_HEAVY_MIN", 0)
    off = build_shard(g, 0, 1)
    assert off.fwd_strips is not None
    assert off.fwd_strip_heavy is None and off.strip_heavy_min == 0


def test_heavy_min_knob_is_pinned(monkeypatch):
    monkeypatch.setattr(partition, "_HEAVY_MIN", None)
    monkeypatch.setenv("ROC_SPMM_HEAVY_MIN", "77")
    assert partition.strip_heavy_min() == 77
    monkeypatch.setenv("ROC_SPMM_HEAVY_MIN", "5")
    assert partition.strip_heavy_min() == 77  # first use wins
