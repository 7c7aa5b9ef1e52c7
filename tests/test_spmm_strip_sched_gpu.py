"""Strip-pass scheduling of the SpMM: the heavy-first schedule and the
fused final bf16 store must not change a single bit.

Which team walks a row, and whether the finished row is rounded by the
last pass or by a separate cast pass, leaves every row's own summation
order alone — so everything here is compared with ``torch.equal``
against the plain strip path (natural sweep, fp32 partials, then
``cast_rowscale``). The comparison against ``ops/reference.py`` uses the
tolerance of ``test_spmm_strips_gpu``.

The graph is ``synthetic_graph`` (3000 rows, mean degree 20) with planted
rows whose strip segments hit the edges of the kernel's cases: lengths 0
and 1, HEAVY_MIN - 1 / HEAVY_MIN / HEAVY_MIN + 1, a 63-edge segment that
walks the whole 16/8/4/1 ladder, and a 1200-edge hub (60x the mean).
Width 800 gives four strips; width 4096 >= N gives one."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from roc_amd.graph import CSRGraph, synthetic_graph
from roc_amd.ops import functional as F
from roc_amd.ops import reference as ref
from roc_amd.parallel import partition
from roc_amd.parallel.partition import (build_shard, build_strip_heavy,
                                        build_strip_plan)

DEV = "cuda:0"
N = 3000
HEAVY_MIN = 24
WIDTHS = [800, 4096]
DIMS = [8, 64, 256, 264]
INT_MAX = 2 ** 31 - 1

# planted rows: edges per 800-wide strip (strips 0..3)
PLANTED = {
    5: [0, 1, HEAVY_MIN - 1, HEAVY_MIN],
    6: [HEAVY_MIN + 1, 0, 1, HEAVY_MIN - 1],
    7: [63, HEAVY_MIN, HEAVY_MIN + 1, 0],   # 63 = 3*16 + 8 + 4 + 1 + 1 + 1
    8: [HEAVY_MIN - 1, 0, 0, 0],            # whole-row lengths around the
    9: [HEAVY_MIN, 0, 0, 0],                # threshold for the one-strip plan
    10: [HEAVY_MIN + 1, 0, 0, 0],
    11: [0, 0, 0, 0],
    2990: [300, 300, 300, 300],             # hub, high index: starts late
}


def _ext():
    from roc_amd import _C
    return _C


def _planted_graph():
    g = synthetic_graph(N, 60000, seed=7)
    rp = g.rowptr.numpy()
    ci = g.colidx.numpy()
    rng = np.random.default_rng(3)
    rows = []
    for r in range(N):
        if r in PLANTED:
            cols = [np.sort(rng.choice(min(800, N - 800 * s), size=k,
                                       replace=False)) + 800 * s
                    for s, k in enumerate(PLANTED[r])]
            rows.append(np.concatenate(cols).astype(np.int32))
        else:
            rows.append(ci[rp[r]:rp[r + 1]])
    rowptr = np.zeros(N + 1, dtype=np.int64)
    np.cumsum([len(c) for c in rows], out=rowptr[1:])
    colidx = np.concatenate(rows).astype(np.int32)
    return CSRGraph(num_nodes=N, num_edges=int(rowptr[-1]),
                    rowptr=torch.from_numpy(rowptr),
                    colidx=torch.from_numpy(colidx))


@pytest.fixture(scope="module")
def planted():
    """Graph, per-width strip plans with their heavy lists (on the GPU),
    and per-D bf16 inputs with the CPU reference, all built once."""
    g = _planted_graph()
    plans = {}
    for w in WIDTHS:
        strips = build_strip_plan(g.rowptr, g.colidx, N, w)
        heavy = build_strip_heavy(strips, HEAVY_MIN)
        plans[w] = ([(a.to(DEV), b.to(DEV)) for a, b in strips],
                    [h.to(DEV) for h in heavy], strips)
    assert len(plans[800][0]) == 4 and len(plans[4096][0]) == 1
    seg = np.stack([np.diff(s[0].numpy()) for s in plans[800][2]])
    for r, want in PLANTED.items():
        assert seg[:, r].tolist() == want
    assert seg[:, 2990].sum() >= 50 * g.num_edges / N
    data = {}
    gen = torch.Generator().manual_seed(11)
    for D in DIMS:
        x = torch.randn(N, D, generator=gen).to(torch.bfloat16)
        data[D] = (x.to(DEV), ref.spmm(x.float(), g.rowptr, g.colidx, N))
    scale = (torch.rand(N, generator=gen) + 0.5).to(DEV)
    return g, plans, data, scale


def _plain_partials(x, strips):
    """fp32 partials after every plain pass (the parent's strip path)."""
    out32 = torch.empty(x.shape[0], x.shape[1], dtype=torch.float32,
                        device=DEV)
    states = []
    for i, (srp, sci) in enumerate(strips):
        _ext().spmm(out32, x, srp, sci, None, None, None, i > 0)
        states.append(out32.clone())
    return states


def _cast(out32, scale):
    out = torch.empty(out32.shape, dtype=torch.bfloat16, device=DEV)
    _ext().cast_rowscale(out, out32, scale)
    return out


def _heavy_variants(strips, heavy, host_strips):
    """(name, per-strip list, threshold): the kernel's contract is that
    the list holds exactly the rows with >= threshold edges."""
    empty = [torch.empty(0, dtype=torch.int32, device=DEV) for _ in strips]
    every = [h.to(DEV) for h in build_strip_heavy(host_strips, 0)]
    assert all(h.numel() == N for h in every)
    return [("empty", empty, INT_MAX), ("all", every, 0),
            ("real", heavy, HEAVY_MIN)]


@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("D", DIMS)
def test_heavy_first_bit_equal(planted, D, width):
    _, plans, data, scale = planted
    strips, heavy, host_strips = plans[width]
    x, _ = data[D]
    want = _plain_partials(x, strips)
    want_bf16 = _cast(want[-1], scale)
    assert all(0 < h.numel() < N for h in heavy)
    last = len(strips) - 1
    for name, lists, hmin in _heavy_variants(strips, heavy, host_strips):
        out32 = torch.empty_like(want[0])
        for i, (srp, sci) in enumerate(strips):
            if i == last:  # both forms of the last pass, from one state
                fin = torch.empty_like(want_bf16)
                _ext().spmm(out32, x, srp, sci, scale, None, None, i > 0,
                            0, 0, lists[i], hmin, fin)
                assert torch.equal(fin, want_bf16), (name, "final")
                if i > 0:  # a final pass leaves the partials alone
                    assert torch.equal(out32, want[i - 1]), (name, "kept")
            _ext().spmm(out32, x, srp, sci, None, None, None, i > 0,
                        0, 0, lists[i], hmin)
            assert torch.equal(out32, want[i]), (name, i)


@pytest.mark.parametrize("with_scale", [False, True])
@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("D", DIMS)
def test_final_store_matches_cast_pass(planted, D, width, with_scale):
    _, plans, data, scale = planted
    strips, _, _ = plans[width]
    x, want_ref = data[D]
    sc = scale if with_scale else None
    states = _plain_partials(x, strips)
    want = _cast(states[-1], sc)
    last = len(strips) - 1
    out32 = states[last - 1].clone() if last > 0 else \
        torch.empty_like(states[0])
    got = torch.empty_like(want)
    srp, sci = strips[last]
    _ext().spmm(out32, x, srp, sci, sc, None, None, last > 0, 0, 0,
                None, 0, got)
    assert torch.equal(got, want)
    # and the whole op through the library path against the CPU reference
    lib = F._strip_spmm(x, strips, N, sc)
    assert torch.equal(lib, want)
    if with_scale:
        want_ref = want_ref * scale.cpu().unsqueeze(1)
    tol = want_ref.abs().max().item() * 2 ** -7 + 1e-2
    assert torch.allclose(lib.cpu().float(), want_ref, atol=tol, rtol=0.02), \
        (lib.cpu().float() - want_ref).abs().max()


@pytest.mark.parametrize("n,D", [(40000, 264), (70000, 256)])
def test_heavy_list_longer_than_the_grid(n, D):
    """Past the 8192-block grid cap (32768 teams at TEAM=64, one per wave;
    65536 at TEAM=32, two per wave) both the list phase and the sweep
    take more than one stride."""
    g = synthetic_graph(n, 3 * n, seed=9)
    host = build_strip_plan(g.rowptr, g.colidx, n, 16384)
    strips = [(a.to(DEV), b.to(DEV)) for a, b in host]
    x = torch.randn(n, D, generator=torch.Generator().manual_seed(2)) \
        .to(torch.bfloat16).to(DEV)
    want = _plain_partials(x, strips)
    for hmin in (0, 3):
        lists = [h.to(DEV) for h in build_strip_heavy(host, hmin)]
        out32 = torch.empty_like(want[0])
        for i, (srp, sci) in enumerate(strips):
            _ext().spmm(out32, x, srp, sci, None, None, None, i > 0, 0, 0,
                        lists[i], hmin)
            assert torch.equal(out32, want[i]), (hmin, i)


def test_scatter_gather_uses_both(planted, monkeypatch):
    """Forward + backward through scatter_gather on forced strips: with
    the heavy lists, without them (knob 0), and the parent's sequence
    written out by hand all agree bit for bit."""
    g, _, data, _ = planted
    D = 64
    monkeypatch.setenv("ROC_SPMM_STRIP_MIN_EDGES", "0")
    monkeypatch.setenv("ROC_SPMM_STRIP_WIDTH", "800")
    monkeypatch.setattr(partition, "_HEAVY_MIN", HEAVY_MIN)
    sh_on = build_shard(g, 0, 1).to(DEV)
    monkeypatch.setattr(partition, "_HEAVY_MIN", 0)
    sh_off = build_shard(g, 0, 1).to(DEV)
    assert sh_on.strip_heavy_min == HEAVY_MIN
    assert len(sh_on.fwd_strip_heavy) == len(sh_on.fwd_strips) == 4
    assert len(sh_on.bwd_strip_heavy) == len(sh_on.bwd_strips)
    assert sh_on.fwd_strip_heavy[0].is_cuda
    assert sh_off.fwd_strip_heavy is None and sh_off.bwd_strip_heavy is None
    x = data[D][0]
    gy = torch.randn(N, D, generator=torch.Generator().manual_seed(5)) \
        .to(torch.bfloat16).to(DEV)
    res = []
    for sh in (sh_on, sh_off):
        xg = x.clone().requires_grad_(True)
        y = F.scatter_gather(xg, sh, dst_scale=sh.rsqrt_deg_local)
        y.backward(gy)
        res.append((y.detach(), xg.grad))
    assert torch.equal(res[0][0], res[1][0])
    assert torch.equal(res[0][1], res[1][1])
    # the parent's path by hand: plain passes, then the cast pass
    y_want = _cast(_plain_partials(x, sh_off.fwd_strips)[-1],
                   sh_off.rsqrt_deg_local)
    gs = torch.empty_like(gy)
    _ext().rowscale(gs, gy, sh_off.rsqrt_deg_local)
    dx_want = _cast(_plain_partials(gs, sh_off.bwd_strips)[-1], None)
    assert torch.equal(res[0][0], y_want)
    assert torch.equal(res[0][1], dx_want)


def test_argument_checks(planted):
    _, plans, data, _ = planted
    strips, heavy, _ = plans[800]
    x = data[64][0]
    srp, sci = strips[0]
    out32 = torch.empty(N, 64, dtype=torch.float32, device=DEV)
    ok = torch.empty(N, 64, dtype=torch.bfloat16, device=DEV)

    def call(heavy_rows=None, final_out=None, out=out32):
        _ext().spmm(out, x, srp, sci, None, None, None, False, 0, 0,
                    heavy_rows, HEAVY_MIN, final_out)

    call(heavy[0], ok)  # the good call
    with pytest.raises(RuntimeError, match="bf16"):
        call(final_out=torch.empty(N, 64, dtype=torch.float32, device=DEV))
    with pytest.raises(RuntimeError, match="shape"):
        call(final_out=torch.empty(N, 32, dtype=torch.bfloat16, device=DEV))
    with pytest.raises(RuntimeError, match="shape"):
        call(final_out=torch.empty(N - 1, 64, dtype=torch.bfloat16,
                                   device=DEV))
    with pytest.raises(RuntimeError, match="int32"):
        call(heavy_rows=heavy[0].long())
    with pytest.raises(RuntimeError, match="strip-pass"):
        call(heavy_rows=heavy[0], out=ok)  # bf16 partials
