"""Degree-ordered strip plan (partition.build_strip_plan_ordered), host
side: the plan holds every row's edges exactly once and in their original
order, so the launch sequence over it performs the same fp32 adds as the
natural plan's.

Graph: 300 rows x 200 sources, width 64 (four strips, the last one 8
wide), sorted columns with duplicate (u, v) edges, and planted degrees
around the light threshold and the kernel's 16/8/4/1 ladder."""
import numpy as np
import pytest
import torch

from roc_amd.graph import CSRGraph
from roc_amd.parallel import partition
from roc_amd.parallel.partition import (build_shard, build_strip_plan,
                                        build_strip_plan_ordered,
                                        strip_rows_skewed)

N, NCOLS, WIDTH = 300, 200, 64
LIGHT = 7
PLANTED = [0, 1, LIGHT - 1, LIGHT, LIGHT + 1, 15, 16, 17, 33, 400]


def _graph():
    rng = np.random.default_rng(5)
    deg = rng.integers(2, 30, size=N)
    deg[10:10 + len(PLANTED)] = PLANTED
    # with replacement: duplicate (u, v) edges; 400 > 200 forces them
    rows = [np.sort(rng.integers(0, NCOLS, size=d)).astype(np.int32)
            for d in deg]
    rowptr = np.zeros(N + 1, dtype=np.int64)
    np.cumsum(deg, out=rowptr[1:])
    return torch.from_numpy(rowptr), torch.from_numpy(np.concatenate(rows))


@pytest.fixture(scope="module")
def graph():
    rp, ci = _graph()
    r = rp.numpy()
    c = ci.numpy()
    assert any((np.diff(c[r[i]:r[i + 1]]) == 0).any() for i in range(N))
    return rp, ci


def _row(rp, ci, i):
    return ci.numpy()[int(rp[i]):int(rp[i + 1])]


def test_perm_is_stable_degree_descending(graph):
    rp, ci = graph
    perm, n_heavy, strips, light = build_strip_plan_ordered(
        rp, ci, NCOLS, WIDTH, LIGHT)
    deg = np.diff(rp.numpy())
    p = perm.numpy()
    assert perm.dtype == torch.int32
    assert sorted(p.tolist()) == list(range(N))
    d = deg[p]
    assert (np.diff(d) <= 0).all()
    same = np.diff(d) == 0
    assert (np.diff(p)[same] > 0).all()  # ties in row order
    assert n_heavy == int((deg >= LIGHT).sum())
    assert d[n_heavy - 1] == LIGHT and d[n_heavy] == LIGHT - 1  # == is heavy
    assert len(strips) == 4
    for srp, _ in strips:
        assert srp.dtype == torch.int64 and srp.numel() == n_heavy + 1
    assert light[0].numel() == N - n_heavy + 1


def test_plan_holds_every_row_in_order(graph):
    rp, ci = graph
    perm, n_heavy, strips, light = build_strip_plan_ordered(
        rp, ci, NCOLS, WIDTH, LIGHT)
    p = perm.numpy()
    for i in range(n_heavy):
        segs = []
        for s, (srp, sci) in enumerate(strips):
            seg = _row(srp, sci, i)
            if seg.size:
                assert seg.min() >= s * WIDTH and seg.max() < (s + 1) * WIDTH
            segs.append(seg)
        assert np.array_equal(np.concatenate(segs), _row(rp, ci, p[i]))
    lrp, lci = light
    for j in range(N - n_heavy):
        assert np.array_equal(_row(lrp, lci, j), _row(rp, ci, p[n_heavy + j]))
    total = sum(sci.numel() for _, sci in strips) + lci.numel()
    assert total == ci.numel()


def test_threshold_extremes(graph):
    rp, ci = graph
    _, n_heavy, strips, light = build_strip_plan_ordered(
        rp, ci, NCOLS, WIDTH, 0)
    assert n_heavy == N and light[1].numel() == 0
    assert light[0].tolist() == [0]
    assert sum(sci.numel() for _, sci in strips) == ci.numel()
    _, n_heavy, strips, light = build_strip_plan_ordered(
        rp, ci, NCOLS, WIDTH, 401)
    assert n_heavy == 0 and len(strips) == 4
    assert all(srp.tolist() == [0] and sci.numel() == 0
               for srp, sci in strips)
    assert light[1].numel() == ci.numel()


def test_unsorted_rows_are_refused(graph):
    rp, ci = graph
    bad = ci.clone()
    a = int(rp[19])  # the 400-edge row
    bad[a], bad[a + 399] = ci[a + 399], ci[a]
    assert not partition.rows_sorted(rp, bad)
    with pytest.raises(AssertionError):
        build_strip_plan_ordered(rp, bad, NCOLS, WIDTH, LIGHT)


def _accumulate(acc, x, rp, ci, rows=None):
    """acc[r] += x[u] edge by edge, as one kernel pass does"""
    for i in range(rp.numel() - 1):
        r = i if rows is None else rows[i]
        for u in _row(rp, ci, i):
            acc[r] += x[u]


@pytest.mark.parametrize("light_deg", [0, LIGHT, 401])
def test_launch_sequence_matches_the_natural_plan(graph, light_deg):
    rp, ci = graph
    D = 8
    x = torch.randn(NCOLS, D, generator=torch.Generator().manual_seed(2))
    want = torch.zeros(N, D)
    for srp, sci in build_strip_plan(rp, ci, NCOLS, WIDTH):
        _accumulate(want, x, srp, sci)
    perm, n_heavy, strips, light = build_strip_plan_ordered(
        rp, ci, NCOLS, WIDTH, light_deg)
    p = perm.tolist()
    got = torch.full((N, D), float("nan"))
    # light pass: from zero, stored through the permutation
    buf = torch.zeros(N - n_heavy, D)
    _accumulate(buf, x, *light)
    got[p[n_heavy:]] = buf
    # heavy region: partials in plan order, the final pass stores permuted
    part = torch.zeros(n_heavy, D)
    for srp, sci in strips:
        _accumulate(part, x, srp, sci)
    got[p[:n_heavy]] = part
    assert torch.equal(got, want)


def test_selection_rule(graph):
    rp, ci = graph
    # planted 400-edge row: > 100 edges in every 64-wide strip
    assert strip_rows_skewed(rp, ci, WIDTH, 100, 0)
    assert not strip_rows_skewed(rp, ci, WIDTH, 10 ** 6, 0)
    assert strip_rows_skewed(rp, ci, WIDTH, 10 ** 6, LIGHT)  # light rows
    # Poisson rows: no heavy segment, nothing below the threshold
    rng = np.random.default_rng(1)
    deg = np.clip(rng.poisson(60, size=N), 40, None)
    rows = [np.sort(rng.integers(0, NCOLS, size=d)).astype(np.int32)
            for d in deg]
    prp = np.zeros(N + 1, dtype=np.int64)
    np.cumsum(deg, out=prp[1:])
    prp, pci = torch.from_numpy(prp), torch.from_numpy(np.concatenate(rows))
    seg_max = max(int(np.diff(s[0].numpy()).max())
                  for s in build_strip_plan(prp, pci, NCOLS, WIDTH))
    assert not strip_rows_skewed(prp, pci, WIDTH, seg_max + 1, 40)
    assert strip_rows_skewed(prp, pci, WIDTH, seg_max, 40)


def test_build_shard_picks_per_csr(monkeypatch):
    """Skewed forward rows get the ordered plan, the Poisson transpose
    keeps the natural one with its heavy lists; knob off or the plan's own
    size guard up: both natural."""
    from roc_amd.graph import synthetic_graph
    g = synthetic_graph(2000, 120000, seed=4)
    t_deg = np.bincount(g.colidx.numpy(), minlength=2000)
    monkeypatch.setenv("ROC_SPMM_STRIP_MIN_EDGES", "0")
    monkeypatch.setenv("ROC_SPMM_STRIP_WIDTH", "500")
    monkeypatch.setenv("ROC_SPMM_SCHEDULE", "degree")
    light = int(t_deg.min())  # no transpose row is light
    heavy_min = int(t_deg.max()) + 1  # nor has it a heavy segment
    assert np.diff(g.rowptr.numpy()).min() < light
    monkeypatch.setattr(partition, "_HEAVY_MIN", heavy_min)
    monkeypatch.setattr(partition, "_LIGHT_DEG", light)
    monkeypatch.setattr(partition, "_STRIP_ORDER", True)
    monkeypatch.setattr(partition, "STRIP_ORDER_MIN_EDGES", 0)
    sh = build_shard(g, 0, 1)
    assert sh.fwd_strip_order is not None and sh.fwd_strip_heavy is None
    ph, pl, lrp, lci = sh.fwd_strip_order
    assert ph.numel() + pl.numel() == 2000
    assert all(srp.numel() == ph.numel() + 1 for srp, _ in sh.fwd_strips)
    assert lrp.numel() == pl.numel() + 1
    assert sum(s[1].numel() for s in sh.fwd_strips) + lci.numel() \
        == g.num_edges
    assert sh.bwd_strip_order is None and len(sh.bwd_strip_heavy) == 4
    assert all(srp.numel() == 2001 for srp, _ in sh.bwd_strips)
    moved = sh.to("cpu")
    assert all(torch.equal(a, b) for a, b in
               zip(moved.fwd_strip_order, sh.fwd_strip_order))
    for off in ({"_STRIP_ORDER": False}, {"STRIP_ORDER_MIN_EDGES": 10 ** 9}):
        for k, v in off.items():
            monkeypatch.setattr(partition, k, v)
        sh = build_shard(g, 0, 1)
        assert sh.fwd_strip_order is None and sh.bwd_strip_order is None
        assert all(srp.numel() == 2001 for srp, _ in sh.fwd_strips)
        monkeypatch.setattr(partition, "_STRIP_ORDER", True)
    # a natural row schedule (community-ordered graph) keeps the natural plan
    monkeypatch.setattr(partition, "STRIP_ORDER_MIN_EDGES", 0)
    monkeypatch.setenv("ROC_SPMM_SCHEDULE", "natural")
    assert build_shard(g, 0, 1).fwd_strip_order is None


def test_knobs_are_pinned(monkeypatch):
    monkeypatch.setattr(partition, "_LIGHT_DEG", None)
    monkeypatch.setattr(partition, "_STRIP_ORDER", None)
    monkeypatch.setenv("ROC_SPMM_LIGHT_DEG", "77")
    monkeypatch.setenv("ROC_SPMM_STRIP_ORDER", "0")
    assert partition.strip_light_deg() == 77
    assert partition.strip_order_on() is False
    monkeypatch.setenv("ROC_SPMM_LIGHT_DEG", "5")
    monkeypatch.setenv("ROC_SPMM_STRIP_ORDER", "1")
    assert partition.strip_light_deg() == 77  # first use wins
    assert partition.strip_order_on() is False
