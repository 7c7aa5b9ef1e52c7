"""The strip SpMM on a degree-ordered plan must not change a single bit.

A row's strip segments in strip order are its edge list in ascending
order and the fp32 partials are exact, so the ordered plan's launches
(light rows in one plain pass, heavy rows in K passes over partials kept
in plan order, stores through the permutation) perform the same fp32 adds
per row as the natural plan with heavy lists and as the one-pass kernel:
everything is compared with ``torch.equal``.

Graph: 600 rows x 2048 sources, width 512 (four strips), degrees planted
around the light threshold and the 16/8/4/1 ladder, and one 2000-edge
row."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from roc_amd.graph import synthetic_graph
from roc_amd.ops import functional as F
from roc_amd.parallel import partition
from roc_amd.parallel.partition import (build_shard, build_strip_heavy,
                                        build_strip_plan,
                                        build_strip_plan_ordered)

DEV = "cuda:0"
N, NCOLS, WIDTH = 600, 2048, 512
LIGHT = 16
HEAVY_MIN = 24
PLANTED = [0, 1, LIGHT - 1, LIGHT, LIGHT + 1, 15, 16, 17, 33, 2000]
DIMS = [64, 256, 520]  # TEAM 8, TEAM 32, TEAM 64 with a second column tile
LIGHT_DEGS = [0, LIGHT, 2001]


def _ext():
    from roc_amd import _C
    return _C


def _dev(plan):
    perm, n_heavy, strips, light = plan
    return ([(a.to(DEV), b.to(DEV)) for a, b in strips],
            [perm[:n_heavy].to(DEV), perm[n_heavy:].to(DEV),
             light[0].to(DEV), light[1].to(DEV)])


@pytest.fixture(scope="module")
def setup():
    rng = np.random.default_rng(5)
    deg = rng.integers(2, 60, size=N)
    deg[10:10 + len(PLANTED)] = PLANTED
    rows = [np.sort(rng.choice(NCOLS, size=d, replace=False)).astype(np.int32)
            for d in deg]
    rowptr = np.zeros(N + 1, dtype=np.int64)
    np.cumsum(deg, out=rowptr[1:])
    rp, ci = torch.from_numpy(rowptr), torch.from_numpy(np.concatenate(rows))
    nat = build_strip_plan(rp, ci, NCOLS, WIDTH)
    heavy = [h.to(DEV) for h in build_strip_heavy(nat, HEAVY_MIN)]
    assert len(nat) == 4 and any(h.numel() for h in heavy)
    nat = [(a.to(DEV), b.to(DEV)) for a, b in nat]
    plans = {t: _dev(build_strip_plan_ordered(rp, ci, NCOLS, WIDTH, t))
             for t in LIGHT_DEGS + [2000]}
    assert plans[0][1][1].numel() == 0          # no light rows
    assert plans[2001][1][0].numel() == 0       # no heavy rows
    assert plans[2000][1][0].tolist() == [19]   # n_heavy == 1: the hub
    gen = torch.Generator().manual_seed(11)
    scale = (torch.rand(N, generator=gen) + 0.5).to(DEV)
    rp_d, ci_d = rp.to(DEV), ci.to(DEV)
    data = {}
    for D in DIMS:
        x = torch.randn(NCOLS, D, generator=gen).to(torch.bfloat16).to(DEV)
        want = {}
        for sc in (None, scale):  # both references, computed once
            one = torch.empty(N, D, dtype=torch.bfloat16, device=DEV)
            _ext().spmm(one, x, rp_d, ci_d, sc, None, None)
            lib = F._strip_spmm(x, nat, N, sc, heavy, HEAVY_MIN)
            assert torch.equal(one, lib)
            want[sc is not None] = lib
        data[D] = (x, want)
    return plans, data, scale, (rp_d, ci_d)


@pytest.mark.parametrize("with_scale", [False, True])
@pytest.mark.parametrize("light_deg", LIGHT_DEGS)
@pytest.mark.parametrize("D", DIMS)
def test_ordered_plan_bit_equal(setup, D, light_deg, with_scale):
    plans, data, scale, _ = setup
    strips, order = plans[light_deg]
    x, want = data[D]
    got = F._strip_spmm(x, strips, N, scale if with_scale else None,
                        order=order)
    assert torch.equal(got, want[with_scale])


@pytest.mark.parametrize("D", [64, 256])
def test_one_heavy_row(setup, D):
    """n_heavy == 1: every strip pass has one row, so every team of the
    grid but one finds nothing to do."""
    plans, data, scale, _ = setup
    strips, order = plans[2000]
    x, want = data[D]
    assert torch.equal(F._strip_spmm(x, strips, N, scale, order=order),
                       want[True])


def test_bad_out_rows_entries_are_skipped(setup):
    plans, data, scale, _ = setup
    strips, order = plans[LIGHT]
    x, want = data[64]
    rows = order[1].clone()
    bad = [0, rows.numel() // 2, rows.numel() - 1]
    lost = rows[bad].long()
    rows[bad[0]], rows[bad[1]], rows[bad[2]] = -1, N, 2 ** 31 - 1
    out = torch.full((N, 64), 7.0, dtype=torch.bfloat16, device=DEV)
    _ext().spmm(out, x, order[2], order[3], scale, None, None, False, 0, 0,
                None, 0, None, rows)
    light = order[1].long()
    keep = torch.ones(N, dtype=torch.bool, device=DEV)
    keep[lost] = False
    ok = light[keep[light]]
    assert torch.equal(out[ok], want[True][ok])
    assert (out[lost] == 7.0).all()             # skipped, not written
    assert (out[order[0].long()] == 7.0).all()  # heavy rows: not this pass
    # the same through a final pass
    hrows = order[0].clone()
    hlost = int(hrows[3])
    hrows[3] = N
    out32 = torch.empty(hrows.numel(), 64, dtype=torch.float32, device=DEV)
    fin = torch.full((N, 64), 7.0, dtype=torch.bfloat16, device=DEV)
    for i, (srp, sci) in enumerate(strips):
        if i < len(strips) - 1:
            _ext().spmm(out32, x, srp, sci, None, None, None, i > 0)
        else:
            _ext().spmm(out32, x, srp, sci, scale, None, None, i > 0, 0, 0,
                        None, 0, fin, hrows)
    hv = order[0].long()
    hv = hv[hv != hlost]
    assert torch.equal(fin[hv], want[True][hv])
    assert (fin[hlost] == 7.0).all()


def test_argument_checks(setup):
    plans, data, scale, (rp_d, ci_d) = setup
    strips, order = plans[LIGHT]
    perm_heavy, perm_light, lrp, lci = order
    x = data[64][0]
    out = torch.empty(N, 64, dtype=torch.bfloat16, device=DEV)
    out32 = torch.empty(perm_heavy.numel(), 64, dtype=torch.float32,
                        device=DEV)
    srp, sci = strips[0]

    def light(rows=perm_light, row_order=None, heavy_rows=None, o=out, xx=x):
        _ext().spmm(o, xx, lrp, lci, None, None, row_order, False, 0, 0,
                    heavy_rows, 0, None, rows)

    def final(rows=perm_heavy, heavy_rows=None, o32=out32):
        _ext().spmm(o32, x, srp, sci, None, None, None, False, 0, 0,
                    heavy_rows, 0, out, rows)

    light()
    final()  # the good calls
    with pytest.raises(RuntimeError, match="int32"):
        light(rows=perm_light.long())
    with pytest.raises(RuntimeError, match="rowptr size"):
        light(rows=perm_light[:-1])
    with pytest.raises(RuntimeError, match="rowptr size"):
        final(rows=perm_heavy[:-1].contiguous())
    with pytest.raises(RuntimeError, match="one entry per row"):
        final(o32=torch.empty(N, 64, dtype=torch.float32, device=DEV))
    with pytest.raises(RuntimeError, match="excludes"):
        light(row_order=torch.arange(perm_light.numel(), dtype=torch.int32,
                                     device=DEV))
    with pytest.raises(RuntimeError, match="excludes"):
        final(heavy_rows=torch.empty(0, dtype=torch.int32, device=DEV))
    with pytest.raises(RuntimeError, match="bf16"):
        light(o=torch.empty(N, 64, dtype=torch.float32, device=DEV),
              xx=x.float())
    with pytest.raises(RuntimeError, match="bf16"):  # fp32 partials, no final
        light(o=torch.empty(N, 64, dtype=torch.float32, device=DEV))
    with pytest.raises(RuntimeError):
        light(rows=perm_light.cpu())


class _Spy:
    """roc_amd._C with its spmm calls recorded"""

    def __init__(self, ext):
        self._ext = ext
        self.calls = []

    def __getattr__(self, name):
        return getattr(self._ext, name)

    def spmm(self, *a, **kw):
        self.calls.append({"out_rows": len(a) > 13 and a[13] is not None,
                           "heavy": len(a) > 10 and a[10] is not None})
        return self._ext.spmm(*a, **kw)


def test_scatter_gather_end_to_end(monkeypatch):
    g = synthetic_graph(3000, 60000, seed=7)
    t_deg = np.bincount(g.colidx.numpy(), minlength=3000)
    monkeypatch.setenv("ROC_SPMM_STRIP_MIN_EDGES", "0")
    monkeypatch.setenv("ROC_SPMM_STRIP_WIDTH", "800")
    monkeypatch.setenv("ROC_SPMM_SCHEDULE", "degree")
    monkeypatch.setattr(partition, "_HEAVY_MIN", HEAVY_MIN)
    monkeypatch.setattr(partition, "_LIGHT_DEG", max(int(t_deg.min()), 1))
    monkeypatch.setattr(partition, "_STRIP_ORDER", True)
    monkeypatch.setattr(partition, "STRIP_ORDER_MIN_EDGES", 0)
    sh_ord = build_shard(g, 0, 1).to(DEV)
    monkeypatch.setattr(partition, "_STRIP_ORDER", False)
    sh_nat = build_shard(g, 0, 1).to(DEV)
    assert sh_ord.fwd_strip_order is not None
    assert sh_ord.fwd_strip_order[1].numel() > 0  # it has light rows
    assert sh_nat.fwd_strip_order is None and sh_nat.bwd_strip_order is None
    spy = _Spy(F._C)
    monkeypatch.setattr(F, "_C", spy)
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(3000, 64, generator=gen).to(torch.bfloat16).to(DEV)
    gy = torch.randn(3000, 64, generator=gen).to(torch.bfloat16).to(DEV)
    res, calls = [], []
    for sh in (sh_ord, sh_nat):
        spy.calls = []
        xg = x.clone().requires_grad_(True)
        y = F.scatter_gather(xg, sh, dst_scale=sh.rsqrt_deg_local)
        fwd_calls = list(spy.calls)
        y.backward(gy)
        res.append((y.detach(), xg.grad))
        calls.append((fwd_calls, spy.calls[len(fwd_calls):]))
    assert torch.equal(res[0][0], res[1][0])
    assert torch.equal(res[0][1], res[1][1])
    k = len(sh_nat.fwd_strips)
    # ordered forward: light pass + K passes, two of them through out_rows
    fwd = calls[0][0]
    assert len(fwd) == k + 1 and not any(c["heavy"] for c in fwd)
    assert [c["out_rows"] for c in fwd] == [True] + [False] * (k - 1) + [True]
    ordered_bwd = sh_ord.bwd_strip_order is not None
    assert any(c["out_rows"] for c in calls[0][1]) == ordered_bwd
    # natural plan: K heavy-first passes, never out_rows
    assert len(calls[1][0]) == k and all(c["heavy"] for c in calls[1][0])
    assert not any(c["out_rows"] for c in calls[1][0] + calls[1][1])
    # fp32 input on the ordered shard: the one-pass kernel, same sums
    spy.calls = []
    y32 = F.scatter_gather(x.float(), sh_ord)
    assert len(spy.calls) == 1 and not spy.calls[0]["out_rows"]
    assert torch.equal(y32, F.scatter_gather(x.float(), sh_nat))


def test_graph_capture(setup):
    plans, data, scale, _ = setup
    strips, order = plans[LIGHT]
    x, want = data[256]
    xs = x.clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        F._strip_spmm(xs, strips, N, scale, order=order)  # warm the allocator
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = F._strip_spmm(xs, strips, N, scale, order=order)
    x2 = torch.randn(NCOLS, 256, generator=torch.Generator().manual_seed(3)) \
        .to(torch.bfloat16).to(DEV)
    eager2 = F._strip_spmm(x2, strips, N, scale, order=order)
    for src, ref in ((x, want[True]), (x2, eager2), (x, want[True])):
        xs.copy_(src)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, ref)
