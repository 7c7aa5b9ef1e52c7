"""The one-pass mean / std / max / min kernels (seg_stats.hip) against the
fp64 CPU reference, and the PNA model on the GPU."""
import pytest
import torch

from roc_amd import (AdamOptimizer, Trainer, build_model, build_shard,
                     pna_delta)
from roc_amd.graph import synthetic_dataset, synthetic_graph
from roc_amd.ops import functional as F
from roc_amd.ops import reference as ref

from test_segstats_cpu import EPS, STATS_NSRC, stats_hand_case

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N = 3000
_CACHE = {}

# fp32: 25x over the 4e-6 the shifted sums measure on the CPU; the
# unshifted form misses it on the offset inputs by two orders of magnitude
TOL32 = dict(rtol=1e-4, atol=1e-6)
# bf16: one rounding (2^-8 relative) with a factor-two margin
TOL16 = dict(rtol=2.0 ** -7, atol=1e-6)


def graph():
    """(cpu shard, gpu shard) of the shared test graph."""
    if "g" not in _CACHE:
        sh = build_shard(synthetic_graph(N, 60000, seed=5), 0, 1)
        _CACHE["g"] = (sh, sh.to(DEV))
    return _CACHE["g"]


def features(D, kind="randn"):
    """bf16-representable fp32 [N, D]: randn, or 100 + 0.25 * randn."""
    key = ("x", D, kind)
    if key not in _CACHE:
        gen = torch.Generator().manual_seed(1 + D)
        x = torch.randn(N, D, generator=gen)
        if kind == "offset":
            x = 100.0 + 0.25 * x
        _CACHE[key] = x.bfloat16().float().contiguous()
    return _CACHE[key]


def expected(D, kind="randn"):
    """(out, stats, arg) of the fp64 reference; computed once per case."""
    key = ("want", D, kind)
    if key not in _CACHE:
        sh, _ = graph()
        _CACHE[key] = ref.seg_stats(features(D, kind).double(), sh.rowptr,
                                    sh.colidx, N, EPS)
    return _CACHE[key]


def close(got, want, tol):
    return torch.allclose(got.double(), want.double(), **tol)


def used(got, want, tol):
    """the worst |got - want| as a fraction of what tol allows there"""
    want = want.double()
    allowed = tol["atol"] + tol["rtol"] * want.abs()
    return float(((got.double() - want).abs() / allowed).max())


def test_graph_properties():
    sh, _ = graph()
    deg = sh.rowptr[1:] - sh.rowptr[:-1]
    assert int(deg.min()) == 1 and int(deg.max()) == 284
    assert int((deg == 1).sum()) == 48
    key = sh.row_of_edge() * N + sh.colidx.long()
    assert key.numel() - key.unique().numel() > 0  # duplicate edges
    t_deg = sh.t_rowptr[1:] - sh.t_rowptr[:-1]
    assert int(t_deg.min()) == 7 and int(t_deg.max()) == 35


@pytest.mark.parametrize("kind", ["randn", "offset"])
@pytest.mark.parametrize("dtype,D", [
    (torch.float32, 4), (torch.float32, 41), (torch.float32, 256),
    (torch.bfloat16, 8), (torch.bfloat16, 40), (torch.bfloat16, 256),
    (torch.bfloat16, 520)])
def test_forward(dtype, D, kind):
    from roc_amd import _C
    _, shg = graph()
    want_out, want_stats, want_arg = expected(D, kind)
    x = features(D, kind).to(dtype).to(DEV)
    out = torch.full((N, 4 * D), 7.0, dtype=dtype, device=DEV)
    stats = torch.full((N, 2 * D), 7.0, dtype=torch.float32, device=DEV)
    arg = torch.full((N, 2 * D), 7, dtype=torch.int32, device=DEV)
    _C.seg_stats_fwd(out, stats, arg, x, shg.rowptr, shg.colidx,
                     shg.row_order, EPS)
    out, stats, arg = out.cpu(), stats.cpu(), arg.cpu()
    assert torch.equal(arg, want_arg)
    assert torch.equal(out[:, 2 * D:], want_out[:, 2 * D:].to(dtype))
    tol = TOL32 if dtype == torch.float32 else TOL16
    got_ms, want_ms = out[:, :2 * D], want_out[:, :2 * D]
    print(f"worst error / tolerance: mean|std {used(got_ms, want_ms, tol):.3f}"
          f", stats {used(stats, want_stats, TOL32):.3f}")
    assert close(got_ms, want_ms, tol)
    assert close(stats, want_stats, TOL32)  # unrounded in both dtypes
    # the op (no gradient: the variant without stats and arg): same bits
    assert torch.equal(F.scatter_gather_stats(x, shg, EPS).cpu(), out)


@pytest.mark.parametrize("dtype,D", [(torch.float32, 6), (torch.float32, 36),
                                     (torch.bfloat16, 7),
                                     (torch.bfloat16, 12),
                                     (torch.bfloat16, 16),
                                     (torch.bfloat16, 136)])
def test_hand_csr(dtype, D):
    """Empty, degree-1, all-equal, all-negative, degree-29 and 100 + small
    rows; row_order given equals None bit for bit (36 fp32 / 136 bf16
    columns put 16 / 32 lanes on a row); 7 bf16 columns are rows without
    4-B alignment, 12 a full unit and a straddling one."""
    from roc_amd import _C
    g, x = stats_hand_case(D)
    want_out, want_stats, want_arg = ref.seg_stats(
        x.double(), g.rowptr, g.colidx, g.n_local, EPS)
    xg = x.to(dtype).to(DEV)
    rp, ci = g.rowptr.to(DEV), g.colidx.to(DEV)
    res = []
    for order in (None, torch.arange(g.n_local - 1, -1, -1, dtype=torch.int32,
                                     device=DEV)):
        out = torch.full((g.n_local, 4 * D), 7.0, dtype=dtype, device=DEV)
        stats = torch.full((g.n_local, 2 * D), 7.0, device=DEV)
        arg = torch.full((g.n_local, 2 * D), 7, dtype=torch.int32, device=DEV)
        _C.seg_stats_fwd(out, stats, arg, xg, rp, ci, order, EPS)
        bare = torch.full((g.n_local, 4 * D), 7.0, dtype=dtype, device=DEV)
        _C.seg_stats_fwd(bare, None, None, xg, rp, ci, order, EPS)
        res.append((out.cpu(), stats.cpu(), arg.cpu(), bare.cpu()))
    tol = TOL32 if dtype == torch.float32 else TOL16
    for out, stats, arg, bare in res:
        assert torch.equal(out, res[0][0]) and torch.equal(stats, res[0][1])
        assert torch.equal(arg, want_arg)
        assert torch.equal(bare, out)  # the variant without stats and arg
        assert torch.equal(out[:, 2 * D:], want_out[:, 2 * D:].to(dtype))
        assert close(out[:, :2 * D], want_out[:, :2 * D], tol)
        assert close(stats, want_stats, TOL32)
        assert torch.equal(out[0], torch.zeros(4 * D, dtype=dtype))
        assert torch.equal(stats[0], torch.zeros(2 * D))
    # backward on the same case: source 8 has no edge and gets zeros
    gen = torch.Generator().manual_seed(D)
    dy = torch.randint(-3, 4, (g.n_local, 4 * D), generator=gen).float()
    xd = x.double().requires_grad_(True)
    F.scatter_gather_stats(xd, g, EPS).backward(dy.double())
    want = xd.grad
    g.rowptr, g.colidx = rp, ci
    g.t_rowptr, g.t_colidx = g.t_rowptr.to(DEV), g.t_colidx.to(DEV)
    xg.requires_grad_(True)
    F.scatter_gather_stats(xg, g, EPS).backward(dy.to(dtype).to(DEV))
    check_grad(xg.grad, want, dtype)
    assert torch.equal(xg.grad[STATS_NSRC - 1].cpu(),
                       torch.zeros(D, dtype=dtype))


def check_grad(got, want, dtype):
    """the tolerances test_layernorm_gpu.py uses for its gradients"""
    assert got.dtype == dtype
    scale = float(want.abs().max())
    if dtype == torch.float32:
        tol = dict(atol=1e-4 * scale, rtol=1e-4)
    else:
        tol = dict(atol=scale * 2.0 ** -7, rtol=0.02)
    err = (got.cpu().double() - want).abs().max()
    print(f"grad max abs err {err:.3e} at scale {scale:.3e}")
    assert torch.allclose(got.cpu().double(), want, **tol), (err, scale)


@pytest.mark.parametrize("dtype,D", [(torch.float32, 41),
                                     (torch.bfloat16, 40),
                                     (torch.bfloat16, 256),
                                     (torch.bfloat16, 520)])
def test_backward(dtype, D):
    """520 columns are 130 four-column units: three column tiles of the
    64-lane team, the last one partly idle."""
    sh, shg = graph()
    gen = torch.Generator().manual_seed(D)
    dy = torch.randint(-3, 4, (N, 4 * D), generator=gen).float()
    xd = features(D).double().requires_grad_(True)
    F.scatter_gather_stats(xd, sh, EPS).backward(dy.double())
    x = features(D).to(dtype).to(DEV).requires_grad_(True)
    out = F.scatter_gather_stats(x, shg, EPS)
    out.backward(dy.to(dtype).to(DEV))
    check_grad(x.grad, xd.grad, dtype)


def test_two_runs_are_bit_identical():
    _, shg = graph()
    D = 40
    dy = torch.randn(N, 4 * D, generator=torch.Generator().manual_seed(3))
    dy = dy.bfloat16().to(DEV)
    runs = []
    for _ in range(2):
        x = features(D).bfloat16().to(DEV).requires_grad_(True)
        out = F.scatter_gather_stats(x, shg, EPS)
        out.backward(dy)
        runs.append((out.detach().cpu(), x.grad.cpu()))
    assert torch.equal(runs[0][0], runs[1][0])
    assert torch.equal(runs[0][1], runs[1][1])


def test_short_x_is_refused():
    _, shg = graph()
    x = features(8).bfloat16().to(DEV)
    with pytest.raises(ValueError):
        F.scatter_gather_stats(x[:-1], shg)


def _pna_trainer():
    g, feats, labels, mask, c = synthetic_dataset("cora", scale=0.3, seed=2)
    pad = (-feats.shape[1]) % 8
    if pad:
        feats = torch.nn.functional.pad(feats, (0, pad))
    shard = build_shard(g, 0, 1)
    model = build_model("pna", [feats.shape[1], 64, c], dropout=0.2, seed=1,
                        delta=pna_delta(g))
    opt = AdamOptimizer(model.parameters(), lr=0.01, weight_decay=1e-4)
    gs = 1.0 / max(int((mask == 1).sum()), 1)
    return Trainer(model, shard, feats, labels, mask, opt, device=DEV,
                   compute_dtype=torch.bfloat16, grad_scale=gs)


def test_pna_trains_gpu():
    tr = _pna_trainer()
    m0 = tr.evaluate()
    for _ in range(30):
        tr.train_epoch()
    m1 = tr.evaluate()
    assert m1["ce_loss"] == m1["ce_loss"], "NaN loss"
    assert m1["ce_loss"] < m0["ce_loss"], (m0, m1)


def test_pna_trains_under_graph_capture():
    """Both launches are capturable: the whole epoch replays as a
    hipGraph."""
    tr = _pna_trainer()
    tr.enable_graph_capture(warmup_epochs=2)
    m0 = tr.evaluate()
    for _ in range(30):
        tr.train_epoch()
    captured = tr._graph is not None
    m1 = tr.evaluate()
    F.set_dropout_counter(None)
    assert captured, "the epoch was never captured"
    assert m1["ce_loss"] == m1["ce_loss"], "NaN loss"
    assert m1["ce_loss"] < m0["ce_loss"], (m0, m1)
